/*
 * restir_c.h -- C ABI of the MI355X-native ReSTIR direct-lighting sampler (libromis_amd.so).
 *
 * Drop-in boundary for the reference's ReSTIR render entry:
 *   renderRayTraced(prevGrid, Scene, Trackball, EmbreeInterface, Screen, Features)   src/rendering/render.cpp:268-290
 *   renderReSTIR   (prevGrid, Scene, Trackball, EmbreeInterface, Screen, Features)   src/rendering/render.cpp:28-62
 * Plain pointers and sizes only: no C++ / torch types cross this line.  The C++ wrapper that keeps the
 * reference's call surface (value-typed grids, exceptions) is include/romis_amd/restir.hpp.
 *
 * Conventions (mirroring the reference):
 *  - every entry point returns restir_status; the message of the last failure on the calling thread is
 *    restir_last_error() (the C++ wrapper rethrows it as std::runtime_error, as render.cpp:99/278 do);
 *  - a context owns one HIP device, one HIP stream and all device buffers; calls on one context are
 *    serialised by the context, different contexts are independent (main.cpp:213-230 renders per thread);
 *  - a restir_frame is the device-resident replacement of std::shared_ptr<ReservoirGrid> (main.cpp:165):
 *    reference-counted, never copied to the host unless downloaded.
 *  - pixel (x, y) uses the reference's convention: y = 0 is the BOTTOM row (render_utils.cpp:24-25); the RGB
 *    image handed back is laid out like Screen's texture (screen.cpp:37-43): row 0 = TOP.
 *
 * Keyed RNG (the parity contract; the reference's rand()/random_device/mt19937 are not seedable):
 *   mix32(h)          = murmur3 fmix32
 *   key(s,f,stage,p)  = mix32(mix32(mix32(s ^ 0x9E3779B9) + f) ^ (stage * 0x01000193 + p * 0x27D4EB2F))
 *   pix(key, g)       = mix32(key ^ mix32(g * 0x9E3779B1 + 0x7F4A7C15))        g = global pixel id y*W + x
 *   draw(pix, slot)   = mix32(pix + slot * 0x9E3779B9)
 *   rand()            -> draw >> 1 ; u = linearMap(float(rand()), 0, RAND_MAX, 0, 1)   (utils.cpp:26-31)
 *   U{0..L-1}         -> (uint64(draw) * L) >> 32
 *   U{-r..r}          -> ((uint64(draw) * (2r+1)) >> 32) - r
 * stages / slots:
 *   RESTIR_STAGE_RIS      (pass 0): candidate c: light 4c, first rand 4c+1, second rand 4c+2, accept 4c+3
 *   RESTIR_STAGE_TEMPORAL (pass 0): accept of the t-th Reservoir::update = t
 *   RESTIR_STAGE_SPATIAL  (pass p): neighbour n: dx 2n, dy 2n+1; accept of the t-th update = 2k + t
 *   R-MIS / R-OMIS (restir_render with RESTIR_MODE_RMIS / ROMIS):
 *   RESTIR_STAGE_RIS      (pass i): the i-th MIS iteration's genInitialSamples, slots as above
 *   RESTIR_STAGE_NEIGHBOURS         generateResampleIndicesGrid (neighbour_selection.cpp:45-122), once per render:
 *     Random strategy (pass 0): candidate n: x 2n, y 2n+1, U{lo..hi} -> lo + ((uint64(draw) * (hi-lo+1)) >> 32)
 *     std::sample over the similar list (pass 0) / the dissimilar list (pass 1): selection sampling, the list's
 *     i-th element is kept iff U{0..len-1-i} (slot i) < the number still needed
 */
#ifndef RESTIR_C_H
#define RESTIR_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RESTIR_ABI_VERSION 5   /* 2: restir_features gained the R-MIS / R-OMIS fields;
                                  3: textures (restir_texture, restir_material.kd_texture, restir_mesh.texcoords);
                                  4: halo passes split into interior / border, native RCCL halo transport,
                                     frame output (8-bit BMP, Features JSON record);
                                  5: the native transport's operation list (restir_halo_ops) and its record-only
                                     mode (restir_halo_record / restir_halo_log) */

#define RESTIR_STAGE_RIS      1u
#define RESTIR_STAGE_TEMPORAL 2u
#define RESTIR_STAGE_SPATIAL  3u
#define RESTIR_STAGE_NEIGHBOURS 4u
#define RESTIR_DEFAULT_SEED   0x5EED0001u
#define RESTIR_MAX_N          32u   /* numSamplesInReservoir slider range 1..32 (ui.cpp:305) */

typedef enum restir_status {
    RESTIR_OK              = 0,
    RESTIR_ERR_INVALID     = 1,  /* bad argument (null pointer, size, range) */
    RESTIR_ERR_HIP         = 2,  /* HIP runtime failure */
    RESTIR_ERR_NO_DEVICE   = 3,  /* no usable gfx950 device */
    RESTIR_ERR_STATE       = 4,  /* call out of order (e.g. render before set_scene) */
    RESTIR_ERR_UNSUPPORTED = 5,  /* feature combination not implemented (e.g. R-OMIS with more than
                                    RESTIR_ROMIS_MAX_TECHNIQUES techniques, or an R-MIS / R-OMIS screen tile handed to
                                    restir_render: restir_render_mis_tile renders those) */
    RESTIR_ERR_COMM        = 6   /* RCCL failure */
} restir_status;

/* RayTraceMode (src/utils/common.h:25-29): renderReSTIR, renderRMIS, renderROMIS (render.cpp:28-265). */
typedef enum restir_mode { RESTIR_MODE_RESTIR = 0, RESTIR_MODE_RMIS = 1, RESTIR_MODE_ROMIS = 2 } restir_mode;
/* MISWeightRMIS (common.h:31-34) and NeighbourSelectionStrategy (common.h:36-41) */
typedef enum restir_mis_weight { RESTIR_MIS_EQUAL = 0, RESTIR_MIS_BALANCE = 1 } restir_mis_weight;
typedef enum restir_neighbour_strategy {
    RESTIR_NEIGHBOURS_RANDOM = 0, RESTIR_NEIGHBOURS_SIMILAR = 1, RESTIR_NEIGHBOURS_DISSIMILAR = 2,
    RESTIR_NEIGHBOURS_EQUAL_SIMILAR_DISSIMILAR = 3
} restir_neighbour_strategy;

/* std::variant<PointLight, SegmentLight, ParallelogramLight> (common.h:72-87) flattened. 88 bytes. */
typedef enum restir_light_type {
    RESTIR_LIGHT_POINT = 0, RESTIR_LIGHT_SEGMENT = 1, RESTIR_LIGHT_PARALLELOGRAM = 2
} restir_light_type;
typedef struct restir_light {
    uint32_t type;
    float p0[3];   /* Point.position | Segment.endpoint0 | Parallelogram.v0     */
    float p1[3];   /*                | Segment.endpoint1 | Parallelogram.edge01 */
    float p2[3];   /*                                    | Parallelogram.edge02 */
    float c0[3];   /* Point.color    | Segment.color0    | Parallelogram.color0 */
    float c1[3];   /*                | Segment.color1    | Parallelogram.color1 */
    float c2[3];   /*                                    | Parallelogram.color2 */
    float c3[3];   /*                                    | Parallelogram.color3 */
} restir_light;

/* Image (framework/include/framework/image.h): width x height texels, row-major [y][x] with y = 0 the image
 * file's first row (Image::pixels order), each texel the stb RGB bytes / 255.0f (image.cpp:22-31). */
typedef struct restir_texture {
    uint32_t     width, height;
    const float* rgb;              /* [height][width][3] */
} restir_texture;

/* Material (framework/include/framework/mesh.h:22-34).  kd_texture = Material::kdTexture: 0 = none, else
 * 1 + an index into restir_set_scene_textured's textures (several materials may share one Image). */
typedef struct restir_material {
    float    kd[3];
    float    ks[3];
    float    shininess;
    float    transparency;
    uint32_t kd_texture;
} restir_material;

/* Mesh (mesh.h:36-43): one material per mesh, like loadMesh's per-material sub-meshes. */
typedef struct restir_mesh {
    const float*    positions;     /* [num_vertices][3] */
    const float*    normals;       /* [num_vertices][3] */
    uint32_t        num_vertices;
    const uint32_t* triangles;     /* [num_triangles][3] vertex indices */
    uint32_t        num_triangles;
    restir_material material;
    const float*    texcoords;     /* [num_vertices][2] Vertex::texCoord; NULL = (0, 0) (loadMesh's default) */
} restir_mesh;

/* Trackball state (framework/include/framework/trackball.h:13-66) as set by Trackball(window, fovy, dist)
 * + setCamera(lookAt, rotation, dist) (main.cpp:223-224). Angles in radians. */
typedef struct restir_camera {
    float fovy;
    float aspect;          /* Window::getAspectRatio() = float(w)/float(h) (window.cpp:380-385) */
    float look_at[3];
    float distance;
    float rotation[3];     /* Euler angles (x, y, z) */
} restir_camera;

/* Derived per-frame camera constants (Trackball::position / generateRay, trackball.cpp:75-78,105-114). */
typedef struct restir_camera_frame {
    float origin[3];
    float quat[4];         /* x, y, z, w of glm::quat(rotation) */
    float half_w, half_h;  /* m_halfScreenSpaceWidth / Height */
} restir_camera_frame;

/* The Features fields read on the ReSTIR path (common.h:89-136). */
typedef struct restir_features {
    uint32_t ray_trace_mode;                 /* restir_mode */
    uint32_t initial_light_samples;          /* M  */
    uint32_t num_samples_in_reservoir;       /* N  (1..RESTIR_MAX_N) */
    uint32_t num_neighbours_to_sample;       /* k  */
    uint32_t spatial_resample_radius;        /* r  */
    uint32_t spatial_resampling_passes;
    uint32_t temporal_clamp_m;
    uint8_t  initial_samples_visibility_check;
    uint8_t  unbiased_combination;
    uint8_t  spatial_reuse;
    uint8_t  spatial_reuse_visibility_check;
    uint8_t  temporal_reuse;
    uint8_t  enable_shading;
    uint8_t  enable_texture_mapping;         /* diffuseAlbedo's switch (utils.cpp:33-37) */
    uint8_t  enable_tone_mapping;
    float    gamma;
    float    exposure;
    /* R-MIS / R-OMIS parameters and the neighbour-selection heuristic (common.h:110-121) -- ABI v2 */
    uint8_t  neighbour_same_geometry;                   /* true */
    uint8_t  use_progressive_romis;                     /* false */
    uint8_t  save_alphas_visualisation;                 /* true; R-OMIS writes the per-distribution bitmaps
                                                           when the context has a renders dir
                                                           (restir_set_renders_dir) */
    uint8_t  reserved0;
    float    neighbour_max_depth_difference_fraction;   /* 0.10 */
    float    neighbour_max_normal_angle_difference_radians; /* 0.436332, compared with the normals' dot product
                                                           as areSimilar does (neighbour_selection.cpp:16-18) */
    uint32_t max_iterations_mis;                        /* 5 */
    uint32_t neighbour_selection_strategy;              /* restir_neighbour_strategy, default SIMILAR */
    uint32_t mis_weight_rmis;                           /* restir_mis_weight, default EQUAL */
    uint32_t progressive_update_mod;                    /* 1 */
} restir_features;

/* Defaults of struct Features (common.h:89-136), rayTraceMode forced to ReSTIR. */
void restir_features_default(restir_features* out);

/* Keyed RNG (see header comment). Exposed for tests and tools. */
uint32_t restir_rng_key(uint32_t seed, uint32_t frame, uint32_t stage, uint32_t pass);
uint32_t restir_rng_draw(uint32_t key, uint32_t global_pixel, uint32_t slot);

/* Host-side camera derivation, identical to the device path's constants. */
void restir_camera_derive(const restir_camera* cam, restir_camera_frame* out);

/* ---- screen tiling (multi-GPU) : pure host logic, callable without a GPU ---------------------------- */
/* Tile (tx, ty) of a tiles_x x tiles_y grid over a global width x height image.  The tile's region is
 * [x0, x0+w) x [y0, y0+h); its ghost region (what a rank must compute locally so that `passes` spatial
 * passes of radius r give bit-identical results to a single-GPU frame) is the region grown by
 * passes*r pixels, clipped to the image. */
typedef struct restir_tile {
    uint32_t global_width, global_height;
    uint32_t x0, y0, width, height;          /* owned pixels */
    uint32_t gx0, gy0, gwidth, gheight;      /* computed pixels (owned + ghost zone) */
} restir_tile;
restir_status restir_tile_plan(uint32_t global_width, uint32_t global_height, uint32_t tiles_x, uint32_t tiles_y,
                               uint32_t rank, uint32_t ghost, restir_tile* out);

/* Reservoir halo exchange between tiles (multi-GPU frames with temporal reuse).  In halo mode a
 * rank computes RIS / temporal / spatial / final only on its owned tile; before every spatial pass the
 * reservoirs within `radius` of a tile border are exchanged with the adjacent ranks.  restir_halo_plan lists,
 * for `rank`, one segment per adjacent rank (ascending rank order): `send[i]` = the rectangle of this rank's
 * owned pixels that rank send[i].rank reads, `recv[i]` = the rectangle of that rank's owned pixels this rank
 * reads.  A segment's bytes = w * h * N * 32, laid out [sub-reservoir j][pixel row-major][res_a, res_b];
 * `offset` is its byte offset in the contiguous send / recv buffer (segments back to back in list order).
 * Pure host; every rank computes the same plan.  *count: in = capacity (>= 8 suffices), out = segments. */
typedef struct restir_halo_segment {
    uint32_t rank;
    uint32_t x0, y0, width, height;          /* global pixel rectangle */
    uint64_t offset, bytes;
} restir_halo_segment;
restir_status restir_halo_plan(uint32_t global_width, uint32_t global_height, uint32_t tiles_x, uint32_t tiles_y,
                               uint32_t rank, uint32_t radius, uint32_t N, restir_halo_segment* send,
                               restir_halo_segment* recv, uint32_t* count);

/* Uneven screen tiles (cost-balanced plans for frames whose geometry is not spread evenly).  A layout
 * cuts the image into tiles_x columns at x_cuts (x_cuts[0] = 0 < x_cuts[1] < ... < x_cuts[tiles_x] = width) and
 * each column c into tiles_y rows at its own y_cuts[c] (0 = y_cuts[c][0] < ... < y_cuts[c][tiles_y] = height); rank
 * ty * tiles_x + tx owns [x_cuts[tx], x_cuts[tx + 1]) x [y_cuts[tx][ty], y_cuts[tx][ty + 1]).  One rectangle per rank,
 * every pixel owned once; with tiles_y <= 4 a rank has at most 2 + 2 tiles_y halo partners (<= 8 segments).  Any
 * layout renders bit-identically to one GPU: the spatial clamp is global (render_utils.cpp:109-110) and the RNG is
 * keyed by global pixel.  restir_layout_even is restir_tile_plan's split; restir_tile_plan / restir_halo_plan /
 * restir_halo_ops / restir_halo_begin are the _layout functions over it. */
#define RESTIR_MAX_TILES_X 16u
#define RESTIR_MAX_TILES_Y 16u
typedef struct restir_tile_layout {
    uint32_t global_width, global_height, tiles_x, tiles_y;
    uint32_t x_cuts[RESTIR_MAX_TILES_X + 1];
    uint32_t y_cuts[RESTIR_MAX_TILES_X][RESTIR_MAX_TILES_Y + 1];
} restir_tile_layout;
restir_status restir_layout_even(uint32_t global_width, uint32_t global_height, uint32_t tiles_x, uint32_t tiles_y,
                                 restir_tile_layout* out);
/* A layout balancing `cost` -- a cost_w x cost_h grid of per-cell work over the image (row-major, row 0 = the bottom
 * row, cell (i, j) = the pixels x with floor(x cost_w / width) = i and y with floor(y cost_h / height) = j, the cell's
 * cost spread evenly over them): the x cuts split the column totals into equal shares, then each column's y cuts
 * split its own row totals.  Cuts are rounded to multiples of align_x / align_y (0: 1) and keep every tile at least
 * one alignment unit wide / high.  *efficiency (may be NULL) = mean over ranks of a rank's cost / the largest. */
restir_status restir_layout_balanced(uint32_t global_width, uint32_t global_height, uint32_t tiles_x, uint32_t tiles_y,
                                     const float* cost, uint32_t cost_w, uint32_t cost_h, uint32_t align_x,
                                     uint32_t align_y, restir_tile_layout* out, double* efficiency);
/* The cost share a layout gives each rank (out[rank], summing to 1) under the same cost grid. */
restir_status restir_layout_shares(const restir_tile_layout* layout, const float* cost, uint32_t cost_w, uint32_t cost_h,
                                   double* out);
restir_status restir_layout_tile(const restir_tile_layout* layout, uint32_t rank, uint32_t ghost, restir_tile* out);
restir_status restir_layout_halo_plan(const restir_tile_layout* layout, uint32_t rank, uint32_t radius, uint32_t N,
                                      restir_halo_segment* send, restir_halo_segment* recv, uint32_t* count);

/* ---- context ----------------------------------------------------------------------------------------- */
/* (halo-mode frame functions: after the render / stage API below) */
typedef struct restir_ctx   restir_ctx;
typedef struct restir_frame restir_frame;

const char*   restir_last_error(void);
int           restir_abi_version(void);
restir_status restir_device_count(int* out);

restir_status restir_create(int device, restir_ctx** out);
void          restir_destroy(restir_ctx* ctx);
restir_status restir_set_seed(restir_ctx* ctx, uint32_t seed, uint32_t frame_index);
/* The reference's RENDERS_DIR (a build-time constant there) for this context's file side outputs; NULL or "" =
 * none (the default).  With a dir, an R-OMIS render with features->save_alphas_visualisation writes
 * visualiseAlphas' bitmaps after every iteration (render.cpp:227-229, render_utils.cpp:189-243):
 * <dir>/<"%d-%m-%Y %H-%M-%S" local time>/Distribution <i> - <Red|Green|Blue>.bmp for technique i of the k + 1,
 * each pixel mix(black, (1, .5, 0), alpha) for alpha > 0 and mix(black, (0, .5, 1), -alpha) otherwise, the
 * alphas solved from the technique matrix and contribution vectors so far -- byte for byte the reference's images
 * (iterations within one second share the folder and overwrite, as there).  The dirs are created as needed;
 * a file that cannot be written fails the render (RESTIR_ERR_INVALID). */
restir_status restir_set_renders_dir(restir_ctx* ctx, const char* dir);

/* Uploads the scene: materials, light SoA table, and the flattened BVH built on the host (replaces
 * EmbreeInterface(scene), embree_interface.cpp:14-51). */
restir_status restir_set_scene(restir_ctx* ctx, const restir_mesh* meshes, uint32_t num_meshes,
                               const restir_light* lights, uint32_t num_lights);
/* The same with the Images textured materials point at (diffuseAlbedo's kdTexture, utils.cpp:33-37): with
 * features->enable_texture_mapping (the Features default, common.h:95) a textured material's diffuse colour
 * is acquireTexel(kdTexture, the hit's interpolated texCoord) (texture.cpp:4-9, embree_interface.cpp:80-81).
 * Texture coordinates outside [0, 1] read out of bounds in the reference (its float -> size_t conversion);
 * here they clamp to the edge texel. */
restir_status restir_set_scene_textured(restir_ctx* ctx, const restir_mesh* meshes, uint32_t num_meshes,
                                        const restir_light* lights, uint32_t num_lights,
                                        const restir_texture* textures, uint32_t num_textures);

/* ---- dynamic scenes: moving geometry and lights between frames without another upload ----
 * New vertex positions (and optionally normals) for meshes of the uploaded scene; the topology -- triangles, vertex
 * counts, materials, textures -- stays.  The device recomputes the triangle records, refits the BVH's boxes over the
 * tree restir_set_scene built and re-quantizes the shadow rays' nodes; nothing is rebuilt on the host.  The tree only
 * prunes, so every later frame equals, bit for bit, the frame a fresh restir_set_scene of the moved scene gives.  A tree
 * refitted far from the scene it was split for walks more nodes per ray: restir_set_scene is the remedy.
 * RESTIR_ERR_STATE before a scene exists; RESTIR_ERR_INVALID (and nothing changes) for a mesh index out of range, a
 * vertex count that is not the upload's, NULL positions, a mesh named twice, or a position that is not finite.  The
 * arrays may be freed on return.  The update is ordered after every frame enqueued so far and before every later one;
 * temporal predecessors stay valid (their samples are lights).  count == 0 does nothing. */
typedef struct restir_mesh_update {
    uint32_t     mesh;          /* index into restir_set_scene's meshes */
    uint32_t     num_vertices;  /* must equal the upload's */
    const float* positions;     /* [num_vertices][3] */
    const float* normals;       /* [num_vertices][3]; NULL = keep the uploaded normals */
} restir_mesh_update;
restir_status restir_update_meshes(restir_ctx* ctx, const restir_mesh_update* updates, uint32_t count);
/* Replaces the light list (any count, any types, or none) and keeps the geometry, the BVH and the kept G-buffer: a still
 * camera over moving lights traces no primary rays.  Everything restir_set_scene derives from the lights is derived
 * again (restir_scene_info reports it).  A temporal predecessor rendered before the call carries its samples' old
 * positions and colours, as the reference's previousFrameGrid does. */
restir_status restir_set_lights(restir_ctx* ctx, const restir_light* lights, uint32_t num_lights);
/* Tests: the device's scene arrays as they stand (any pointer NULL = skip).  Sizes from restir_scene_info: nodes
 * 8 floats per node, nodes_q 4 words per node (untouched when !nodes_q_ok), triangle records 4 floats per triangle --
 * v0 / e1 / e2 in BVH order, n0 / n1 / n2 in the upload's order. */
restir_status restir_debug_scene_download(restir_ctx* ctx, float* nodes, uint32_t* nodes_q, float* tri_v0, float* tri_e1,
                                          float* tri_e2, float* tri_n0, float* tri_n1, float* tri_n2);

/* renderRayTraced (render.cpp:268-290) by features->ray_trace_mode:
 * RMIS / ROMIS -- renderRMIS / renderROMIS (render.cpp:64-265): primary hits -> neighbour selection grid ->
 * max_iterations_mis x (initial RIS -> per-pixel MIS combination over the pixel's neighbourhood) -> screen.
 * Whole images only here (tile NULL or covering the image; any other tile is RESTIR_ERR_UNSUPPORTED --
 * restir_render_mis_tile renders screen tiles), no temporal predecessor, *out_next = NULL (the reference
 * returns std::nullopt).  R-OMIS needs k + 1 <= RESTIR_ROMIS_MAX_TECHNIQUES and at least k candidates in every
 * pixel's window (the reference indexes past the neighbourhood otherwise).
 * RESTIR -- renderReSTIR (render.cpp:28-62): primary hits -> initial RIS -> [temporal if prev] -> [spatial x P] ->
 * final shading + tone map.  `prev` may be NULL (no temporal predecessor).  `out_next` (nullable) receives
 * a new reference to the frame's final reservoir grid.  `out_rgb` (nullable, host, width*height*3 floats,
 * row 0 = top) -- when NULL the call only enqueues work and returns without synchronising; the image stays
 * on the device (restir_download_rgb).  `tile` (nullable) restricts the frame to one screen tile of a
 * larger image (multi-GPU); NULL = the whole width x height image.  A tiled frame's grid is defined on the owned
 * rect: its ghost ring (computed only for the owned pixels' spatial neighbourhoods) holds intermediate values. */
restir_status restir_render(restir_ctx* ctx, const restir_camera* cam, const restir_features* features,
                            uint32_t width, uint32_t height, const restir_tile* tile,
                            const restir_frame* prev, restir_frame** out_next, float* out_rgb);

/* R-MIS / R-OMIS on screen tiles (multi-GPU frames, and frames whose whole-image buffers would not fit; DESIGN.md
 * §7, §10).  A pixel's neighbourhood lies within spatial_resample_radius r of it, and every neighbour contributes only
 * its own G-buffer record and its own RIS reservoir of the iteration, both keyed by global pixel: a tile that computes
 * primary rays and RIS on its owned rectangle grown by r (clipped to the image) reproduces its owned pixels bit for bit,
 * for any number of iterations, with no exchange between ranks and no state between frames.
 *
 * restir_render_mis_tile: renderRMIS / renderROMIS of the owned rectangle of `tile`.  out_rgb (nullable, as
 * restir_render's): tile->width x tile->height x 3 floats, row 0 = top of the tile.  tile == NULL: the whole image (the
 * bits of restir_render in these modes).  ray_trace_mode must be RMIS or ROMIS (RESTIR_ERR_INVALID otherwise); the tile
 * must be consistent (as restir_render's) and its computed region must hold the owned rectangle grown by r on every
 * side, clipped to the image (RESTIR_ERR_INVALID; restir_tile_plan / restir_layout_tile with ghost = r give such tiles).
 * The R-OMIS window rule and the neighbourhood capacity are the global image's.  One frame index is consumed per call:
 * after restir_set_seed(seed, f) a tile's owned pixels are the whole-image render's after the same call.  The G-buffer,
 * reservoir and debug planes are sized by the computed region; neighbourhoods, accumulators, per-sample scratch and the
 * image by the owned rectangle.  save_alphas_visualisation with a renders dir set is RESTIR_ERR_UNSUPPORTED on a tile
 * that is not the whole image (the bitmaps are whole-image files). */
restir_status restir_render_mis_tile(restir_ctx* ctx, const restir_camera* cam, const restir_features* features,
                                     uint32_t width, uint32_t height, const restir_tile* tile, float* out_rgb);
/* Every tile of `layout` in turn on this context (rank 0 .. n - 1, restir_layout_tile with ghost = r), all with ONE
 * frame index (consumed once), stitched into the whole image out_rgb (global_width x global_height x 3 floats, row 0 =
 * top): frames whose whole-image buffers would not fit.  Fails on the first tile that fails. */
restir_status restir_render_mis_tiles(restir_ctx* ctx, const restir_camera* cam, const restir_features* features,
                                      const restir_tile_layout* layout, float* out_rgb);

/* ---- motion-compensated temporal reuse: a predecessor grid reprojected to another camera --------------------
 * restir_render combines pixel p with the predecessor's pixel p (temporalReuse, render_utils.cpp:142-177), which is
 * right while the camera stands still.  restir_frame_reproject gathers a NEW predecessor grid for a camera that moved:
 * *out (of prev's size and N) holds at every pixel the N sub-reservoirs of `prev` at the pixel where the current
 * camera's surface point was seen from cam_prev, or empty reservoirs (all-zero words); hand it to
 * restir_render(..., prev = *out, ...) as `prev` would be, and release it like any frame.  The call consumes no frame
 * index and draws no random number, leaves `prev` untouched (it orders itself after prev's producer and records its
 * read, as a render does), and never touches the kept G-buffer ("gbuf.reuse"): it traces both cameras into scratch
 * planes of its own, so the next restir_render traces again.  Per pixel p = (x, y), y = 0 the bottom row:
 *   1. (N_cur, t_cur, P, material) = the G-buffer record of cam_cur at p; a primary-ray miss -> empty (reason 0);
 *   2. v = P - o_prev, c = conj(q_prev) * v (quat * vec3); !(c.z > 0) -> empty (1, behind the camera);
 *   3. r = c.x / c.z, nx = (-r) / half_w, s = c.y / c.z, ny = s / half_h,
 *      fx = floorf(((nx + 1) * 0.5f) * W + 0.5f), fy likewise with ny and H -- the nearest sample position, single
 *      float32 operations in this order; !(0 <= fx < W && 0 <= fy < H) (NaN included) -> empty (2, off-screen);
 *   4. (n_prev, t_prev, material) = the record of cam_prev at q = (fx, fy), traced over the geometry AS IT STANDS NOW
 *      (after restir_update_meshes a moved mesh is validated against its new place); a miss -> empty (3);
 *   5. d = glm::length(v); fabsf(1 - t_prev / d) > 0.1f -> empty (4, depth), else dot(n_prev, N_cur) < 0.90630778703f
 *      -> empty (5, normal): render_utils.cpp:114-118 with the current depth replaced by d, whatever
 *      unbiased_combination says;
 *   6. otherwise prev's sub-reservoirs at q, bit for bit.
 * When prev carries frame handles ("spatial.handles") they are gathered too -- an empty pixel gets the zero sample's
 * handle (W = 0, M = 0, the light count as index) -- so the fused handle-reading temporal kernel still runs.
 * out_map (nullable, host, W * H words): the flat index fy * W + fx of q, or 0xFFFFFFFF - reason for an empty pixel;
 * with it the call synchronises, without it it only enqueues.  With timing enabled the two primary-ray launches count
 * under RESTIR_K_PRIMARY; the gather itself is not timed.
 * RESTIR_ERR_INVALID: a NULL argument, a predecessor on another device, a camera whose derived frame is not finite;
 * RESTIR_ERR_STATE: before a scene is set; RESTIR_ERR_UNSUPPORTED: a predecessor that is a screen tile (its view is not
 * the whole image) or in the per-pixel records layout ("layout.records").
 *
 * restir_reproject_pixel (pure host): steps 2-3 for one point P and the predecessor's derived camera -- the kernel's
 * own text (csrc/reproject.h), bit for bit.  *x, *y = the source pixel, or both 0xFFFFFFFF - reason (1 or 2);
 * *depth (nullable) = d of step 5.  RESTIR_ERR_INVALID for a NULL argument (depth aside) or W * H == 0. */
restir_status restir_frame_reproject(restir_ctx* ctx, const restir_frame* prev, const restir_camera* cam_prev,
                                     const restir_camera* cam_cur, restir_frame** out, uint32_t* out_map);
restir_status restir_reproject_pixel(const restir_camera_frame* prev_cam, uint32_t W, uint32_t H, const float P[3],
                                     uint32_t* x, uint32_t* y, float* depth);

restir_status restir_frame_retain(restir_frame* frame);
/* Drops a reference.  The last one hands the grid's device records back to the producing context for re-use,
 * ordered on the GPU after every kernel that wrote or read them (no host or device-wide synchronisation). */
void          restir_frame_release(restir_frame* frame);

/* The grid a frame holds -- renderReSTIR's returned ReservoirGrid (render.h:25-28, render.cpp:61) -- over the
 * frame's computed view (vw x vh pixels at (vx0, vy0) of the W x H image; the whole image for untiled frames).
 * restir_frame_info: any pointer may be NULL.  restir_frame_download copies, per sub-reservoir j and view pixel
 * p (index j * vw * vh + p, rows y = 0 bottom): outputSamples[j].position -> pos[3 i], .color -> color[3 i],
 * .W -> w[i], sampleNums[j] -> m[i]; any output may be NULL, each holds vw * vh * N entries (x3 for pos /
 * color).  Waits for the frame's producer, then copies synchronously. */
restir_status restir_frame_info(const restir_frame* frame, uint32_t* width, uint32_t* height, uint32_t* vx0,
                                uint32_t* vy0, uint32_t* vw, uint32_t* vh, uint32_t* n);
restir_status restir_frame_download(const restir_frame* frame, float* pos, float* color, float* w, uint32_t* m);
restir_status restir_synchronize(restir_ctx* ctx);

/* Last rendered image (owned pixels), host float RGB, row 0 = top. */
restir_status restir_download_rgb(restir_ctx* ctx, float* out_rgb, size_t count);

/* ---- presenting a frame: snapshots of the last image through a pinned, pipelined read-back ------------------
 * The last rendered image (what restir_download_rgb serves: float3 per owned pixel, row 0 = top) converted on the
 * device and copied into pinned host memory without stalling the frames behind it.  Formats:
 *   RESTIR_IMAGE_RGB32F           the floats themselves, 12 bytes per pixel, bit for bit
 *   RESTIR_IMAGE_RGBA8            restir_rgb_to_rgba8's bytes (Screen::writeBitmapToFile's conversion), 4 per pixel
 *   RESTIR_IMAGE_BGRA8_BOTTOM_UP  the same bytes as stbi_write_bmp's pixel body: B, G, R, A, the last image row first
 *                                 (a BMP file = the header + this buffer)
 * restir_image_begin takes one of the context's RESTIR_MAX_IMAGES_IN_FLIGHT slots -- a device staging buffer and a
 * pinned host buffer, created on first need, grown for a larger image, kept for re-use, freed by restir_destroy --,
 * enqueues the conversion (RGB32F: a device-to-device copy) on the context's stream behind the frame that produced
 * the image, then the device-to-host copy on the context's copy stream (created by the first restir_image_begin)
 * behind the conversion, and returns without synchronising anything.  The snapshot lives in staging: the next
 * restir_render may overwrite the image at once, and only the copy -- not the frames enqueued after it -- is waited
 * for.  restir_image_ready never blocks; restir_image_wait blocks until this snapshot's copy has landed and returns
 * the pinned bytes (restir_image_info's `bytes` of them), valid until restir_image_release, which waits for the copy
 * if it has not landed and frees the slot for re-use (NULL: no-op).
 * RESTIR_ERR_STATE: nothing rendered yet, or RESTIR_MAX_IMAGES_IN_FLIGHT snapshots unreleased; RESTIR_ERR_INVALID: a
 * NULL argument or an unknown format.  restir_destroy waits for the outstanding copies and frees the slots: handles
 * still unreleased are invalid afterwards and must not be used, not even released.  A handle belongs to its context
 * and is used from one thread at a time, like the context.  Between restir_halo_begin and restir_halo_end the image
 * has its size but not yet its pixels: a snapshot taken there holds undefined content (as restir_download_rgb would).
 * restir_download_rgba8: begin(RGBA8), wait, memcpy, release -- `pixels` = the capacity of out_rgba in pixels
 * (RESTIR_ERR_INVALID when below the image's).  restir_write_image_bmp: the last image as the file restir_write_bmp
 * writes from its floats, from a BGRA8_BOTTOM_UP snapshot (RESTIR_ERR_INVALID when the file cannot be written).
 * The conversion launch has no RESTIR_K_* slot: restir_timings does not see it. */
typedef enum restir_image_format { RESTIR_IMAGE_RGB32F = 0, RESTIR_IMAGE_RGBA8 = 1,
                                   RESTIR_IMAGE_BGRA8_BOTTOM_UP = 2 } restir_image_format;
typedef struct restir_image restir_image;
#define RESTIR_MAX_IMAGES_IN_FLIGHT 4u
restir_status restir_image_begin(restir_ctx* ctx, uint32_t format, restir_image** out);
restir_status restir_image_info(const restir_image* image, uint32_t* width, uint32_t* height, uint32_t* format,
                                size_t* bytes);   /* any out pointer may be NULL */
restir_status restir_image_ready(restir_image* image, int* ready);
restir_status restir_image_wait(restir_image* image, const void** data);
void          restir_image_release(restir_image* image);
restir_status restir_download_rgba8(restir_ctx* ctx, uint8_t* out_rgba, size_t pixels);
restir_status restir_write_image_bmp(restir_ctx* ctx, const char* path);

/* ---- accumulating frames: running mean, variance and converged image on the device -------------------------
 * A context folds its last image -- what restir_download_rgb serves, 3 floats per owned pixel -- into a running mean
 * and, with RESTIR_ACCUM_VARIANCE, a sum of squared deviations m2, one of each per float, without the image leaving
 * the device.  Folding the n-th image value x (n = 1, 2, ...) uses inv_n = 1.0f / (float)n computed once on the host and
 * three single float32 operations without contraction, in this order (Welford's recurrence with a reciprocal):
 *     d = x - mean;   mean' = mean + d * inv_n;   m2' = m2 + d * (x - mean')
 * IEEE special values propagate as the operations give them; a NaN's payload and sign are not part of the contract.
 * Tone map AFTER averaging: render the frames with enable_tone_mapping = 0 and hand the tone-mapping fields to
 * restir_accum_resolve (the mean of tone-mapped frames is biased dark).
 *   restir_accum_begin      starts (or restarts) an accumulation with an empty state; the buffers -- 12 bytes per pixel, 24
 *                           with the variance -- are created by the first add
 *   restir_accum_add        folds the last image in; it only enqueues, on the context's stream behind the frame
 *   restir_accum_resolve    writes the mean as the context's last image, tone mapped by tone's enable_tone_mapping /
 *                           gamma / exposure with the final kernels' own arithmetic (tone == NULL: the mean's bits);
 *                           restir_download_rgb, restir_image_begin, restir_download_rgba8 and restir_write_image_bmp
 *                           then serve the resolved image.  It only enqueues and leaves the state as it is
 *   restir_accum_stats_get  (needs the variance and two frames) synchronises the context's stream: est_mse = the mean
 *                           over the finite floats of m2 / (n (n - 1)), the estimate of E|mean - expectation|^2 per
 *                           float; mean_value = the mean of their means; nonfinite = the floats whose mean or m2 is
 *                           not finite, left out of both.  Deterministic: a fixed two-stage reduction in double
 *   restir_accum_download   test hook: the state as it stands, 3 W H floats each (m2 may be NULL; zeros are written
 *                           for an accumulation without the variance); synchronises
 *   restir_accum_end        closes the accumulation and frees the buffers (restir_destroy does so too)
 *   restir_accum_fold       pure host: the same step over arrays, x folded into mean (and m2) as the n-th value -- the
 *                           kernel's own text, bit for bit; for clients that fold tiles on the CPU
 * An add folds an image a producer wrote -- restir_render, restir_render_mis_tile(s), restir_halo_end, restir_stage_final,
 * restir_stage_mis_finish, or a restir_stage_upload of RESTIR_BUF_RGB -- and each such image once.  It is
 * RESTIR_ERR_STATE, with nothing changed, when no accumulation is open, nothing has been rendered, a halo frame is
 * between restir_halo_begin and restir_halo_end, the last image is a resolve's or was added already, its size is not
 * the accumulation's (the first added image's), or RESTIR_ACCUM_MAX_FRAMES are folded.  restir_accum_resolve without a
 * frame and restir_accum_stats_get with fewer than two, or without the variance, are RESTIR_ERR_STATE; a NULL argument,
 * unknown flags, restir_accum_fold with n = 0 or n > RESTIR_ACCUM_MAX_FRAMES, and a download whose count is below
 * 3 W H are RESTIR_ERR_INVALID.  An allocation the device refuses is RESTIR_ERR_HIP and closes the accumulation.
 * No accumulation call touches the still view's caches (the kept G-buffer, the shadow lists, the visibility bits, the
 * p-hat table, their streak): a view that stands still keeps them while it accumulates.  The launches have no
 * RESTIR_K_* slot: restir_timings does not see them. */
#define RESTIR_ACCUM_VARIANCE   1u
#define RESTIR_ACCUM_MAX_FRAMES 16777215u   /* 2^24 - 1: (float)n is exact */
typedef struct restir_accum_stats {
    uint32_t width, height, frames, flags;
    uint64_t nonfinite;   /* floats left out */
    double   est_mse;     /* sum of terms / floats counted: estimate of E|mean - expectation|^2 per float */
    double   mean_value;  /* sum of mean / floats counted */
} restir_accum_stats;
restir_status restir_accum_begin(restir_ctx* ctx, uint32_t flags);
restir_status restir_accum_add(restir_ctx* ctx);
restir_status restir_accum_resolve(restir_ctx* ctx, const restir_features* tone /* nullable */);
restir_status restir_accum_stats_get(restir_ctx* ctx, restir_accum_stats* out);
restir_status restir_accum_download(restir_ctx* ctx, float* mean, float* m2 /* nullable */, size_t count);
restir_status restir_accum_end(restir_ctx* ctx);
restir_status restir_accum_fold(float* mean, float* m2 /* nullable */, const float* x, size_t count, uint32_t n);

/* "Render until it is good enough" in one call: begins a fresh accumulation (req->flags), then renders frames of one
 * view by restir_render with enable_tone_mapping forced to 0 and adds each, with no host synchronisation between
 * frames.  Every frame consumes its own frame index; with features->temporal_reuse each frame's grid is the next
 * frame's predecessor (the first has none).  With req->target_mse > 0 (needs RESTIR_ACCUM_VARIANCE and check_every > 0,
 * else RESTIR_ERR_INVALID) it takes the stats -- which synchronises -- after frame min_frames and then every check_every
 * frames, and stops once est_mse <= target_mse (a check that cannot be taken yet, with one frame, counts as not
 * met), or at max_frames.  Then it resolves with the caller's tone-mapping fields and fills out_stats (nullable; zeros
 * but for the size, the frame count and the flags where the stats cannot be taken) and out_rgb (nullable, the resolved
 * image as restir_render hands images back).  The accumulation stays open: the caller may add more or read the state.
 * RESTIR_ERR_INVALID: max_frames == 0 or above RESTIR_ACCUM_MAX_FRAMES, min_frames > max_frames, unknown flags.  R-MIS /
 * R-OMIS render whole images; `tile` follows restir_render's rules. */
typedef struct restir_accum_request {
    uint32_t flags, min_frames, max_frames, check_every;
    double   target_mse;
} restir_accum_request;
restir_status restir_render_accumulate(restir_ctx* ctx, const restir_camera* cam, const restir_features* features,
                                       uint32_t width, uint32_t height, const restir_tile* tile,
                                       const restir_accum_request* req, restir_accum_stats* out_stats /* nullable */,
                                       float* out_rgb /* nullable */);

/* ---- the exact direct-lighting image, a kept reference and error figures against it -------------------------
 * restir_render_exact writes, as the context's image, what every estimator here estimates: per owned pixel, with px the
 * G-buffer record of `cam` at that pixel exactly as restir_stage_primary gives it,
 *     color = (+0, +0, +0)
 *     for i = 0 .. L-1, in light-table order:
 *         sc = computeShading(features, px, light[i].position, light[i].colour)       shading.cpp:7-34
 *         if (!testVisibilityLightSample(px.P, light[i].position)) sc = (+0, +0, +0)
 *         color = color + sc                                     three float32 adds, no contraction
 *     if (features->enable_tone_mapping) color = exposureToneMapping(color)          tone_mapping.cpp:8-11
 *     rgb[(rect.h - 1 - (y - rect.y0)) * rect.w + (x - rect.x0)] = color             row 0 = top, as final shading
 * That is, float32-added in light order, L runs of final shading (render.cpp:45-57) with N = 1, tone mapping off and
 * every pixel's reservoir set to (position of light i, colour of light i, W = 1, M = 1): 0 + sc 1, / 1 and the running
 * sum never produce -0, so the bits agree.  A miss pixel follows the same rule (whatever computeShading returns for the
 * miss material); a scene with no lights gives the tone-mapped +0 image; enable_shading = 0 follows computeShading (kd per
 * visible light).  Of `features` only enable_shading, enable_texture_mapping, enable_tone_mapping, gamma and exposure
 * are read: ray_trace_mode and every sampling field are ignored.
 * Scope: scenes whose lights are all point lights, or that have none, with any L.  A scene with a segment or
 * parallelogram light is RESTIR_ERR_UNSUPPORTED with a message naming the light type -- an area light's integral is not
 * a finite sum --, nothing is rendered and the last image is unchanged.  `tile` as restir_render's; the image is
 * pixel-local, so a tile computes exactly its owned rectangle, with no ghost ring, and stitched tiles are the whole
 * image bit for bit.  Between restir_halo_begin and restir_halo_end the call is RESTIR_ERR_STATE.
 * The call is a producer: it writes the context's image and takes a new serial in the accumulator's rule above, so
 * restir_accum_add, restir_image_begin, restir_download_rgb / _rgba8 and restir_write_image_bmp serve it; with
 * out_rgb == NULL it only enqueues.  It consumes no frame index and draws no random number, and neither reads nor
 * writes the kept G-buffer, the tile flags, the shadow lists, the visibility bits, the p-hat table or their streak: it
 * traces its own G-buffer into scratch planes of its own.  Like restir_render it leaves the stage API unconfigured (the
 * image buffer has the tile's size now).  Its launches have no RESTIR_K_* slot.
 * Errors: a NULL argument or an inconsistent tile (RESTIR_ERR_INVALID), a call before restir_set_scene or inside a halo
 * frame (RESTIR_ERR_STATE) and an unsupported scene are found before anything is written and leave the last image as it
 * was.  An allocation or a launch the device refuses (RESTIR_ERR_HIP) comes later and may leave the image buffer, as a
 * frame that failed half way does, with its size but not its pixels: nothing serves or adds it until a producer writes it. */
restir_status restir_render_exact(restir_ctx* ctx, const restir_camera* cam, const restir_features* features,
                                  uint32_t width, uint32_t height, const restir_tile* tile /* nullable */,
                                  float* out_rgb /* nullable, as restir_render's */);

/* A kept reference: restir_reference_set keeps a device copy of the last image -- any producer's, or a resolve's --, 12
 * bytes per owned pixel; it only enqueues.  The copy is a snapshot: later renders, scene updates, new lights and
 * accumulations leave it alone; clearing or replacing it is the caller's call.  Which domain it is in, linear or tone
 * mapped, is the caller's choice: for RESTIR_ERROR_SRC_ACCUM_MEAN render it with enable_tone_mapping = 0, the mean is
 * linear.
 * restir_error_get compares a source with the reference on the device and synchronises; nothing leaves the device but
 * the struct.  Per float, with a the source's and r the reference's value and d = (double)a - (double)r: a float whose
 * a or r is not finite is left out and counted in `nonfinite`; over the others mse, mae, rel_mse and bias are the means
 * of d d, |d|, d d / (r r + RESTIR_ERROR_REL_EPS) and d, max_abs the exact maximum of |d|, ref_mean the mean of r (0 / 0
 * where nothing is counted).  The reduction is deterministic -- block b of 4096 floats, sixteen entries per lane added
 * in index order in double, a fixed tree over the block's lanes, the blocks' partials added in index order on the
 * host; no float atomics -- and restir_error_measure (pure host) is the same arithmetic over two arrays, bit for bit.
 * Every error leaves all state untouched.  RESTIR_ERR_STATE: restir_reference_set without a produced or resolved image, or
 * between restir_halo_begin and restir_halo_end; restir_error_get without a reference, with a source that is absent (no
 * image; no open accumulation or no frame in it) or whose size is not the reference's.  RESTIR_ERR_INVALID: a NULL
 * argument, an unknown source, count == 0.  RESTIR_ERR_HIP: an allocation the device refuses. */
#define RESTIR_ERROR_SRC_IMAGE      0u   /* the context's last image */
#define RESTIR_ERROR_SRC_ACCUM_MEAN 1u   /* the open accumulation's mean (linear: compare with a reference rendered without tone mapping) */
#define RESTIR_ERROR_REL_EPS        1e-2 /* relative MSE's denominator: r*r + eps */
typedef struct restir_error_stats {
    uint32_t width, height, source, frames;   /* frames: the accumulation's count, 0 for SRC_IMAGE */
    uint64_t counted, nonfinite;              /* floats compared / left out because a or r is not finite */
    double   mse, mae, rel_mse, bias;         /* means over the counted floats of d*d, |d|, d*d/(r*r+eps), d;  d = (double)a - (double)r */
    double   max_abs;                         /* max |d| over the counted floats, exact */
    double   ref_mean;                        /* mean of r over the counted floats */
} restir_error_stats;
restir_status restir_reference_set(restir_ctx* ctx);     /* keep a device copy of the last image (any producer, or a resolve) as the reference; enqueues */
restir_status restir_reference_clear(restir_ctx* ctx);   /* frees it; restir_destroy does so too */
restir_status restir_reference_info(restir_ctx* ctx, uint32_t* width, uint32_t* height, int* present);
restir_status restir_error_get(restir_ctx* ctx, uint32_t source, restir_error_stats* out);   /* synchronises */
restir_status restir_error_measure(const float* a, const float* r, size_t count, restir_error_stats* out);   /* pure host, same arithmetic */

/* ---- denoising the last image: an edge-avoiding a-trous wavelet filter guided by the G-buffer ---------------
 * restir_denoise filters the context's last image in place (Dammertz et al. 2010, geometry terms only: no colour or
 * luminance term).  Every step below is one float32 operation without contraction, divide and sqrt correctly rounded;
 * restir_denoise_host (pure host) is the same arithmetic over arrays, bit for bit.
 * Inputs: the image c (w x h float3, row 0 = top) and the G-buffer of the same rectangle exactly as
 * restir_stage_primary gives it: n_t = (N unnormalised, t), p_mat = (P, bits(material)), row y = 0 at the bottom -- the
 * image row of G-buffer row y is h - 1 - y.
 * Per pixel, once:  l2 = (N.x N.x + N.y N.y) + N.z N.z;  the pixel is flat when its material is the miss material
 * (num_materials - 1), or !(l2 > 0), or l2 is not finite;  otherwise g = N / sqrt(l2), component by component.
 * Levels i = 0 .. iterations - 1 with step s = 2^i, each reading the level before.  For pixel p:
 *     sw = +0, sc = (+0, +0, +0)
 *     for dy = -2 .. 2 (image rows), for dx = -2 .. 2:   q = p + s (dx, dy),  h = k[dy] k[dx],  k = (1/16, 1/4, 3/8, 1/4, 1/16)
 *         q outside the image, or c_q with a component that is not finite: skipped
 *         q == p:  w = h                                          (no edge term: sw >= 9/64)
 *         else:    skipped unless material(q) == material(p) as 32-bit patterns;
 *                  both flat: w = h;  exactly one flat: skipped;  neither:
 *                      cn = (g_p.x g_q.x + g_p.y g_q.y) + g_p.z g_q.z;  cn = cn > 0 ? cn : 0;  cn = cn cn, normal_power_log2 times
 *                      d = P_q - P_p;  e = (g_p.x d.x + g_p.y d.y) + g_p.z d.z
 *                      inv_s = 1.0f / (sigma_plane t_p);  r = e inv_s;  wp = 1.0f - r r;  w = h (cn wp)
 *                  skipped unless w > 0 (a NaN fails the test)
 *         sw = sw + w;  sc.j = sc.j + w c_q.j
 *     out.j = sc.j / sw
 * A pixel whose own colour is not finite keeps its input's bits at every level.  After the last level restir_denoise
 * applies exposureToneMapping (the final kernels' own) when `tone` asks for it; of `tone` only enable_tone_mapping, gamma
 * and exposure are read, NULL is no tone mapping.  The viewer's loop: render with enable_tone_mapping = 0, denoise with
 * the tone fields, present.  restir_denoise_host has no tone-mapping step; its `out` must not overlap its inputs.
 * The image is any producer's (a frame, an exact image, an upload of RESTIR_BUF_RGB) or a resolve's, an earlier
 * restir_denoise's included.  `tile` follows restir_render_exact's rules; the owned rectangle must have the image's size.
 * Taps outside the owned rectangle are skipped like taps outside the image: an image denoised tile by tile differs from
 * the whole image's within 2 (2^iterations - 1) pixels of a seam.
 * The result is marked like restir_accum_resolve's: downloads, presentation, restir_write_image_bmp,
 * restir_reference_set, restir_error_get(RESTIR_ERROR_SRC_IMAGE) and another restir_denoise serve it, restir_accum_add
 * refuses it (RESTIR_ERR_STATE).  With out_rgb == NULL the call only enqueues.
 * Towards frame state the call behaves like restir_render_exact: it traces its own guides into scratch planes of its
 * own, consumes no frame index and neither reads nor writes the kept G-buffer, the tile flags, the shadow lists, the
 * visibility bits, the p-hat table or their streak; it leaves the stage API unconfigured; its launches have no
 * RESTIR_K_* slot.  The guides are kept and reused while the camera, width, height, tile and the scene's geometry are
 * unchanged: restir_set_scene and restir_update_meshes drop them, restir_set_lights does not;
 * restir_denoise_guide_builds counts the traces.
 * Errors are found before anything is written and leave the image as it was.  RESTIR_ERR_INVALID: a NULL argument (ctx,
 * camera, params), parameters out of range, an inconsistent tile.  RESTIR_ERR_STATE: no scene, no image, an owned
 * rectangle that has not the image's size, a call between restir_halo_begin and restir_halo_end. */
#define RESTIR_DENOISE_MAX_ITERATIONS 5u
typedef struct restir_denoise_params {
    uint32_t iterations;         /* 1 .. RESTIR_DENOISE_MAX_ITERATIONS; the filter's reach is 2 (2^iterations - 1) pixels.  The default is 2:
                                  * at 1920 x 1080 a third level blurs the lighting itself and every error figure rises again
                                  * (README "Denoising a frame") */
    uint32_t normal_power_log2;  /* 0 .. 7: the normal term is max(g_p . g_q, 0)^(2^normal_power_log2) */
    float    sigma_plane;        /* finite, > 0: the plane term's support as a fraction of the view distance t */
    uint32_t flags;              /* 0 */
} restir_denoise_params;
void restir_denoise_params_default(restir_denoise_params* out);   /* 2, 5, 0.01f, 0 */
restir_status restir_denoise(restir_ctx* ctx, const restir_camera* cam, uint32_t width, uint32_t height,
                             const restir_tile* tile /* nullable */, const restir_denoise_params* params,
                             const restir_features* tone /* nullable */, float* out_rgb /* nullable */);
restir_status restir_denoise_host(const float* rgb, const float* n_t, const float* p_mat, uint32_t w, uint32_t h,
                                  uint32_t miss_material, const restir_denoise_params* params, float* out);   /* pure host, same arithmetic */
restir_status restir_denoise_guide_builds(restir_ctx* ctx, uint64_t* out);   /* guide traces so far, restir_denoise_lum's included */

/* ---- denoising with a variance-guided luminance term ---------------------------------------------------------
 * restir_denoise_lum is restir_denoise with one more factor per tap: a rational luminance weight whose scale is the
 * pixel's own measured noise (after SVGF, Schied et al. 2017, with 1 / (1 + r r) in place of exp(-r): no expf).  A
 * per-pixel variance plane travels through the levels next to the colour.  Every step below is one float32 operation
 * without contraction, divide and sqrt correctly rounded, fabsf exact; restir_denoise_lum_host (pure host) is the same
 * arithmetic over arrays, bit for bit.  Guides, flat rule, k, h, g_p, P, t, material: restir_denoise's, above.
 * Luminance:  l(c) = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b.
 * clean(v) = v when v > 0 and v is finite, else +0: every entry of the initial variance plane v (one float per pixel,
 * image rows) is stored through it.
 * RESTIR_DENOISE_VAR_ACCUM: the input colour is the open accumulation's mean, exactly the bits restir_accum_resolve(ctx,
 *   NULL) would write, whatever the last image is; it needs an open accumulation with RESTIR_ACCUM_VARIANCE, n >= 2 frames
 *   and the owned rectangle's size, else RESTIR_ERR_STATE and nothing changed.  With inv = 1.0f / ((float)n (float)(n - 1)),
 *   computed once on the host:  s.j = sqrtf(m2.j inv) per channel;  sl = l(s);  v = clean(sl sl).  The channels' standard
 *   errors are added, not their variances: the three channels of a ReSTIR sample share one contribution weight, so their
 *   noise is correlated and the luminance's deviation is the weighted sum of the channels'.  The accumulation is read
 *   only: its state, its count and the still view's caches are untouched.
 * RESTIR_DENOISE_VAR_SPATIAL: the input colour is the last image, under restir_denoise's rules.  For a centre p whose
 *   colour is finite:
 *     s0 = s1 = s2 = +0;  inv_s = 1.0f / (geo.sigma_plane t_p)
 *     for dy = -3 .. 3 (image rows), for dx = -3 .. 3:   q = p + (dx, dy)
 *         q outside the rectangle, or c_q with a component that is not finite: skipped
 *         q == p:  w = 1.0f
 *         else:    w = restir_denoise's geometry weight of the tap with h = 1.0f (its material and flat rules
 *                  included: a tap they skip has w = 0);  skipped unless w > 0
 *         l_q = l(c_q);  s0 = s0 + w;  s1 = s1 + w l_q;  s2 = s2 + w (l_q l_q)
 *     m1 = s1 / s0;  v = clean(s2 / s0 - m1 m1)
 *   A centre whose colour is not finite has v = +0.
 * Levels i = 0 .. geo.iterations - 1 with step s = 2^i, each reading the colour and the variance of the level before.
 * For a pixel p whose colour is finite:
 *     gn = gd = +0
 *     for dy = -1 .. 1, for dx = -1 .. 1 (unit offsets at every level):   q = p + (dx, dy), skipped outside the rectangle
 *         gw = g[dy] g[dx],  g = (1/4, 1/2, 1/4);  gn = gn + gw v_q;  gd = gd + gw
 *     gv = gn / gd;  inv_den = 1.0f / (sigma_lum sqrtf(gv) + 1e-6f);  l_p = l(c_p)
 *     sw = +0, sc = (+0, +0, +0), sv = +0
 *     the 25 taps of restir_denoise in its order, its skip rules unchanged, the centre's w = h;  for every other tap
 *         w_geo = restir_denoise's w (0 where its material or flat rule skips the tap)
 *         r = fabsf(l(c_q) - l_p) inv_den;  wl = 1.0f / (1.0f + r r);  w = w_geo wl
 *         skipped unless w > 0 (an infinite r gives wl = 0, a NaN fails the test)
 *     per contributing tap:  sw = sw + w;  sc.j = sc.j + w c_q.j;  sv = sv + (w w) v_q
 *     out.j = sc.j / sw;  v_out = sv / (sw sw)         (v_out is stored as computed, not through clean)
 * A pixel whose own colour is not finite keeps its colour's bits and its v at every level; its v is read by its
 * neighbours' gv like any other.  After the last level restir_denoise_lum applies the tone map as restir_denoise does;
 * the host function has none.
 * restir_denoise_lum_host: var == NULL runs the SPATIAL estimate, otherwise var is the initial plane (w x h floats, image
 * rows), read through clean; params->variance_source is checked and otherwise ignored.  A caller that wants ACCUM's plane
 * computes it from restir_accum_download.  out_var (nullable) receives the last level's variance plane; the outputs must
 * not overlap the inputs.
 * State: the call uses restir_denoise's guide planes and their key -- a view traced by one call is not traced again by the
 * other, restir_denoise_guide_builds counts both.  The result is marked like restir_denoise's; tiles, halo frames, NULL
 * arguments, range errors and the frame state follow restir_denoise's rules.  RESTIR_ERR_INVALID in addition: an unknown
 * variance_source, a sigma_lum that is not a positive finite number, flags != 0, geo out of range.  Errors are found
 * before anything is written.  restir_denoise_lum_variance_download copies the last successful call's final variance
 * plane (count >= W H floats, else RESTIR_ERR_INVALID; no such call since the planes were last dropped: RESTIR_ERR_STATE)
 * and synchronises: a test hook. */
#define RESTIR_DENOISE_VAR_SPATIAL 0u   /* variance estimated from the image itself */
#define RESTIR_DENOISE_VAR_ACCUM   1u   /* image = the open accumulation's mean, variance from its m2 */
typedef struct restir_denoise_lum_params {
    restir_denoise_params geo;   /* as restir_denoise's; geo.flags == 0 */
    uint32_t variance_source;    /* RESTIR_DENOISE_VAR_* */
    float    sigma_lum;          /* finite, > 0: the luminance term's support in standard deviations.  The default stays 4, with geo's 2
                                  * levels, after the sweep of {1, 2, 4, 8} x 1 .. 5 levels at 1920 x 1080: 2 leaves one C2 frame's
                                  * MSE above restir_denoise's (0.649 against 0.485, 4: 0.471); 8 is level with 4 on one frame and
                                  * loses on every mean (16 frames: MSE 0.257 against 0.179) (README "Denoising with a luminance
                                  * term") */
    uint32_t flags;              /* 0 */
} restir_denoise_lum_params;
void restir_denoise_lum_params_default(restir_denoise_lum_params* out);   /* restir_denoise's defaults, SPATIAL, 4.0f, 0 */
restir_status restir_denoise_lum(restir_ctx* ctx, const restir_camera* cam, uint32_t width, uint32_t height,
                                 const restir_tile* tile /* nullable */, const restir_denoise_lum_params* params,
                                 const restir_features* tone /* nullable */, float* out_rgb /* nullable */);
restir_status restir_denoise_lum_host(const float* rgb, const float* var /* nullable: the spatial estimate */, const float* n_t,
                                      const float* p_mat, uint32_t w, uint32_t h, uint32_t miss_material,
                                      const restir_denoise_lum_params* params, float* out_rgb, float* out_var /* nullable */);
restir_status restir_denoise_lum_variance_download(restir_ctx* ctx, float* var, size_t count);   /* the last call's final variance plane; synchronises */

/* ---- a reprojected image history: accumulating while the camera moves ----------------------------------------
 * restir_accum_* folds pixel p into pixel p and so needs a still view.  The history keeps, per pixel, a mean, the
 * population variance S of the samples and a sample count n, and every restir_history_advance moves them to the new
 * camera before it folds the last image in: the temporal half of SVGF (Schied et al. 2017).  restir_history_denoise runs
 * restir_denoise_lum's levels over the mean with a variance plane taken from S.  Every step below is one float32
 * operation without contraction, divide and sqrt correctly rounded; the pure host functions are the kernels' own text
 * (csrc/history.h), bit for bit.
 * Record.  Per pixel: (N unnormalised, t) as the G-buffer's n_t holds it, the material's bits clamped to the miss material
 * (every index at or above it is a miss), mean.rgb, S.rgb and n.  Two sets of three 16-byte planes, 96 bytes per pixel,
 * 190 MiB at 1920 x 1080, allocated by the first advance and freed by restir_history_end.
 * Rows.  G-buffer records -- n_t, p_mat, kept_n_t, kept_material, and the map with the indices in it -- are in G-buffer
 * rows (y = 0 at the bottom) like restir_frame_reproject's; the image, mean, S, n and the variance plane are in image rows
 * (row 0 = top).  Image row r is G-buffer row h - 1 - r.
 * Advance, per pixel p of the new view, whose current record (N, t, P, material) is the new camera's G-buffer record:
 *   1. restir_frame_reproject's steps 1 - 5 with reasons 0 - 5 unchanged.  The predecessor's camera is the camera of the
 *      advance before; the predecessor's record at the source pixel q is the one the history kept from that advance --
 *      nothing is traced a second time.
 *   2. reason 6 (material), tested after reason 5: the kept material at q differs from the current one.
 *   3. reason 7 (no history), tested last: the kept record at q has n == 0.  On the first advance after
 *      restir_history_begin and the first after a reset nothing is kept and every pixel is reason 7, the misses included.
 *   4. On any reason the gathered state is the empty one, (mean, S, n) = (+0, +0, 0); otherwise the kept one at q.
 *   5. The fold of x, the last image at p.  When all of x.rgb are finite:  n' = min(n + 1, max_frames);
 *      a = 1.0f / (float)n';  per channel  d = x - mean;  mean' = mean + d a;  dd = d d;  t = a dd;  u = S + t;
 *      om = 1.0f - a;  S' = om u.  Below the cap mean' is restir_accum_fold's mean, the same operations, and S' is its
 *      m2 / n; with the cap reached both are exponential averages with alpha = 1 / max_frames.  When a component of x is
 *      not finite the gathered state passes through; an empty one then takes x's bits as its mean with S = +0 and n' = 0,
 *      which the next advance treats as empty (reason 7).
 *   6. (N, t, material of the current record, mean', S', n') are stored at p of the other set.
 * out_map (nullable, host, W H words) follows restir_frame_reproject's convention: the flat G-buffer-row index of q, or
 * 0xFFFFFFFF - reason.  With it the call synchronises; without, it only enqueues.
 * The image follows restir_accum_add's producer rules: it must be an image a producer wrote, each is folded once, a
 * resolve's or a denoiser's result and a halo frame are refused.  The "folded already" mark is the history's own: one
 * image may go to restir_accum_add and to restir_history_advance.  cam is the camera the image was rendered with.  The
 * current records come from restir_denoise's guide planes: a view is traced once across restir_history_advance,
 * restir_denoise and restir_denoise_lum, and restir_denoise_guide_builds counts it.  The call consumes no frame index,
 * leaves the image, the kept G-buffer, the tile flags, the shadow lists, the visibility bits, the p-hat table and the RIS
 * look-ahead untouched, and has no RESTIR_K_* slot.  Whole images only: a last image whose size is not width x height (a
 * screen tile's) is RESTIR_ERR_UNSUPPORTED.
 * restir_history_resolve writes the mean (tone mapped by `tone`, or its bits) as the context's image, marked like
 * restir_accum_resolve's.  restir_history_denoise is restir_denoise_lum over the mean -- exactly resolve(NULL)'s bits,
 * whatever the last image is -- for the last advance's view; params->variance_source is checked and otherwise ignored.
 * Its initial variance plane: a pixel whose mean is finite and whose n >= spatial_below has
 *     inv = 1.0f / (float)(n - 1);  v = restir_denoise_lum's ACCUM expression with m2 = S  (s.j = sqrtf(S.j inv), ...)
 * and every other pixel RESTIR_DENOISE_VAR_SPATIAL's estimate at p over the mean image with params->geo.  Under a reached
 * cap S / (n - 1) over-states an exponential average's variance of the mean, by up to about 2 x (the steady-state factor
 * is a / (2 - a) of S); the bias is conservative.  The result is marked like restir_denoise's and
 * restir_denoise_lum_variance_download serves its final plane.  The host equivalent is restir_denoise_lum_host(mean,
 * var = restir_history_variance_host(...)).
 * Resets.  restir_set_scene (and _textured) and restir_update_meshes empty the history -- the kept records describe
 * geometry that has moved --: the next advance is all reason 7, resolve and denoise are RESTIR_ERR_STATE until then, and
 * `resets` counts it.  The size stays.  restir_set_lights does not reset: the history then lags the lighting by about
 * max_frames frames.
 * Errors, all found before anything is written.  RESTIR_ERR_INVALID: a NULL argument, max_frames outside 1 ..
 * RESTIR_ACCUM_MAX_FRAMES, spatial_below < 2, flags or reserved != 0, an empty size, a camera whose derived frame is not
 * finite, a download buffer below W H pixels, a map entry outside the image (restir_history_fold).  RESTIR_ERR_STATE: no
 * scene, no open history, no image, a halo frame, a size other than the history's (the first advance's), an image folded
 * already, a resolved or denoised image, resolve / denoise / download before the first advance (or the first after a
 * reset).  RESTIR_ERR_HIP: an allocation the device refuses; it closes the history.
 * restir_history_map_host: kept_n_t, kept_material and kept_n all NULL describe a history with nothing kept (all reason 7).
 * restir_history_download is a test hook (each of mean, S, n nullable) and synchronises.
 * Tuning "history.var_fused" (1, the default: one launch writes the mean image and the variance plane, running the spatial
 * estimate only for the pixels that take it; 0: the spatial estimate over the whole mean image, the history's entries
 * written over it, three launches): the same bits either way; the knob touches no frame and keeps the still view's caches. */
typedef struct restir_history_params {
    uint32_t max_frames;     /* 1 .. RESTIR_ACCUM_MAX_FRAMES: the count's cap, alpha's floor 1 / max_frames.  The default is 8 after the
                              * sweep of {8, 16, 32, 64} x spatial_below {2, 4, 8} at 1920 x 1080 under a 0.1 degree per frame yaw: the
                              * source pixel is the nearest one, so every advance displaces the history by up to half a pixel and a
                              * longer history drifts further -- at frame 64 the filtered C2 result has MSE 0.233 / rel_mse 0.0021 at
                              * 8, 0.346 / 0.0177 at 16, 0.620 / 0.117 at 32, 0.846 / 0.201 at 64; spatial_below does not separate
                              * (README "Image history") */
    uint32_t spatial_below;  /* >= 2: pixels with fewer samples take the spatial variance estimate */
    uint32_t flags;          /* 0 */
    uint32_t reserved;       /* 0 */
} restir_history_params;
void          restir_history_params_default(restir_history_params* out);   /* 8, 4, 0, 0 */
restir_status restir_history_begin(restir_ctx* ctx, const restir_history_params* params);
restir_status restir_history_advance(restir_ctx* ctx, const restir_camera* cam, uint32_t width, uint32_t height,
                                     uint32_t* out_map /* nullable, host, W*H words: synchronises when given */);
restir_status restir_history_resolve(restir_ctx* ctx, const restir_features* tone /* nullable */);
restir_status restir_history_denoise(restir_ctx* ctx, const restir_denoise_lum_params* params,
                                     const restir_features* tone /* nullable */, float* out_rgb /* nullable */);
restir_status restir_history_download(restir_ctx* ctx, float* mean, float* S, uint32_t* n, size_t pixels);
restir_status restir_history_frames(restir_ctx* ctx, uint64_t* advances, uint64_t* resets);
restir_status restir_history_end(restir_ctx* ctx);
/* pure host, the kernel's own text */
restir_status restir_history_fold(const float* mean_in, const float* S_in, const uint32_t* n_in, const uint32_t* map,
                                  const float* x, uint32_t w, uint32_t h, uint32_t max_frames,
                                  float* mean_out, float* S_out, uint32_t* n_out);
restir_status restir_history_map_host(const restir_camera_frame* prev_cam, uint32_t w, uint32_t h,
                                      const float* cur_n_t, const float* cur_p_mat,
                                      const float* kept_n_t, const uint32_t* kept_material, const uint32_t* kept_n,
                                      uint32_t miss_material, uint32_t* map);
restir_status restir_history_variance_host(const float* mean, const float* S, const uint32_t* n,
                                           const float* n_t, const float* p_mat, uint32_t w, uint32_t h,
                                           uint32_t miss_material, const restir_history_params* params,
                                           const restir_denoise_params* geo, float* var);

/* The gather of restir_history_advance.  NEAREST (the default) takes the kept record of the nearest source pixel, as
 * described above.  BILINEAR blends the 2 x 2 kept records around the continuous source position, SVGF's footprint with a
 * test per tap, so that an advance no longer displaces the history by up to half a pixel:
 *   1. Reasons 0 - 2 are unchanged, the range test on the nearest pixel included: they mark the same pixels in both modes.
 *   2. (cfx, cfy) is the position the nearest pixel is rounded from, cfx = ((nx + 1.0f) * 0.5f) * (float)W; pixel x sits at
 *      coordinate x.  x0 = floorf(cfx); fx = cfx - x0; gx = 1.0f - fx; the same for y.
 *   3. Taps j = 0 .. 3 at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), G-buffer coordinates, with w0 = gx gy,
 *      w1 = fx gy, w2 = gx fy, w3 = fx fy.  A tap contributes when it lies inside the image, w_j > 0 and the kept record
 *      there passes steps 1's tests 3 - 5 and reasons 6 and 7 against the same d.
 *   4. No tap contributes: the pixel is rejected with the reason the nearest pixel gives.  The nearest pixel is one of the
 *      four, so every pixel NEAREST accepts from a given kept state BILINEAR accepts too, and a pixel both reject has the
 *      same reason.
 *   5. sum = the contributing w_j added in tap order; v_j = w_j / sum; per channel mean = sum_j v_j mean_j and
 *      S = sum_j (v_j v_j) S_j, accumulated in tap order from the first term; nf = sum_j v_j (float)n_j,
 *      n = (uint32_t)floorf(nf + 0.5f), raised to 1 from 0.  One contributing tap: its record verbatim.
 *   6. The fold and the stored record are unchanged.
 *   7. out_map: the flat index of the nearest pixel when it contributes, else of the contributing tap of the largest
 *      weight (the first in tap order on a tie); 0xFFFFFFFF - reason for a rejected pixel.
 * What S means afterwards.  restir_history_denoise reads S / (n - 1) as the variance of the kept mean.  A blend of
 * independent means with weights v_j has variance sum_j v_j^2 S_j / (n_j - 1), with equal counts (sum_j v_j^2 S_j) / (n - 1).
 * After a BILINEAR advance S is therefore the number whose S / (n - 1) estimates the variance of the mean, no longer the
 * population variance of the samples; the fold continues from it.  The rule ignores the correlation the blend creates
 * between neighbouring pixels.  The plain average sum_j v_j S_j was tried in a CPU prototype: it made the filtered result
 * worse than this rule.
 * The mode is context state: it may be set at any time, with or without an open history, holds for every later advance
 * until set again -- across restir_history_begin / _end and across resets --, touches no frame and keeps the still view's
 * caches.  Consecutive advances may use different modes: the state planes are the same.  A value above 1 or a NULL
 * argument is RESTIR_ERR_INVALID and changes nothing.
 * restir_history_advance_host is one whole advance in either mode, rows as restir_history_map_host's and
 * restir_history_fold's: with NEAREST exactly those two in sequence.  kept_n_t and kept_material both NULL: nothing kept
 * (mean_in, S_in and n_in are still required, and not read).  n_in is the kept count, image rows.  The outputs must not
 * overlap the inputs.  RESTIR_ERR_INVALID, before anything is written: a NULL argument, one kept pointer without the
 * other, an empty or too large size, max_frames outside 1 .. RESTIR_ACCUM_MAX_FRAMES, gather above 1, with BILINEAR an
 * n_in above RESTIR_ACCUM_MAX_FRAMES. */
typedef enum restir_history_gather { RESTIR_HISTORY_GATHER_NEAREST = 0, RESTIR_HISTORY_GATHER_BILINEAR = 1 } restir_history_gather;
restir_status restir_history_gather_set(restir_ctx* ctx, uint32_t gather);
restir_status restir_history_gather_get(restir_ctx* ctx, uint32_t* gather);
/* pure host, the kernel's own text: one whole advance in either mode */
restir_status restir_history_advance_host(const restir_camera_frame* prev_cam, uint32_t w, uint32_t h,
                                          const float* cur_n_t, const float* cur_p_mat,
                                          const float* kept_n_t, const uint32_t* kept_material,   /* both NULL: nothing kept */
                                          const float* mean_in, const float* S_in, const uint32_t* n_in,
                                          const float* x, uint32_t miss_material, uint32_t max_frames, uint32_t gather,
                                          float* mean_out, float* S_out, uint32_t* n_out, uint32_t* out_map /* nullable */);

/* ---- stage-level access for parity tests and profiling ---------------------------------------------- *
 * Buffers are the device SoA layout (DESIGN.md "Data layout"), one entry per pixel of the computed region
 * (row-major, y = 0 bottom), and for reservoirs [N][pixels]:
 *   gbuf_n_t   : float4 (N.xyz, t)         gbuf_p_mat : float4 (P.xyz, bits(material index))
 *   res_a      : float4 (light pos.xyz, W) res_b      : float4 (light colour.xyz, bits(M))
 *   res_dbg    : float2 (wSum, chosenSampleWeight)
 *   gbuf_uv    : float2 (the hit's interpolated texCoord; written and read only for scenes with textures) */
typedef enum restir_buffer {
    RESTIR_BUF_GBUF_N_T   = 0,   /* read by the spatial heuristic for every neighbour: keep it compact */
    RESTIR_BUF_GBUF_P_MAT = 1,
    RESTIR_BUF_RES_A      = 2,   /* reservoir slot 0 ("current") */
    RESTIR_BUF_RES_B      = 3,
    RESTIR_BUF_RES_DBG    = 4,
    RESTIR_BUF_PREV_A     = 5,   /* reservoir slot 1 (temporal predecessor / spatial ping-pong) */
    RESTIR_BUF_PREV_B     = 6,
    RESTIR_BUF_PREV_DBG   = 7,
    RESTIR_BUF_RGB        = 8,   /* float3 per owned pixel, row 0 = top */
    /* R-MIS / R-OMIS stage buffers (restir_stage_neighbours / restir_stage_mis_accumulate):
     *   mis_nbr : uint32 [1 + cap][pixels]: row 0 = neighbourhood size c, rows 1..c = the neighbourhood's pixel
     *             indices y * width + x, the pixel itself first (cap = restir_stage_mis_capacity)
     *   mis_acc : float [rows][pixels].  R-MIS: colour sum (3 rows).  R-OMIS with T = k + 1: technique matrix A
     *             (T*T rows, element (i, j) in row i + j*T), contribution vectors b (3*T rows, colour c, technique
     *             i in row T*T + c*T + i), progressive alphas (3*T rows after b, same order), progressive colour
     *             (3 rows) */
    RESTIR_BUF_MIS_NBR    = 9,
    RESTIR_BUF_MIS_ACC    = 10,
    RESTIR_BUF_GBUF_UV    = 11
} restir_buffer;
#define RESTIR_ROMIS_MAX_TECHNIQUES 8u   /* k + 1 distributions per pixel (the technique matrix lives in registers) */

/* Allocates stage buffers for a width x height region with N sub-reservoirs (idempotent). */
restir_status restir_stage_configure(restir_ctx* ctx, uint32_t width, uint32_t height, uint32_t n);
restir_status restir_stage_upload(restir_ctx* ctx, restir_buffer which, const void* host, size_t bytes);
restir_status restir_stage_download(restir_ctx* ctx, restir_buffer which, void* host, size_t bytes);

/* Individual passes on the stage buffers (the camera supplies the ray origin every pass shades from).
 * `debug` != 0 also writes the (wSum, chosenSampleWeight) buffer of the pass output.
 *   primary  : -> GBUF_*                         ris      : GBUF -> RES_*
 *   temporal : RES_* (current) + PREV_* -> RES_*
 *   spatial  : ONE pass, RES_* -> new RES_* (the input becomes PREV_*); call once per pass with that
 *              pass's key restir_rng_key(seed, frame, RESTIR_STAGE_SPATIAL, pass)
 *   final    : RES_* -> RGB                                                                                */
restir_status restir_stage_primary(restir_ctx* ctx, const restir_camera* cam);
restir_status restir_stage_ris(restir_ctx* ctx, const restir_camera* cam, const restir_features* f, uint32_t rng_key,
                               int debug);
restir_status restir_stage_temporal(restir_ctx* ctx, const restir_camera* cam, const restir_features* f,
                                    uint32_t rng_key, int debug);
restir_status restir_stage_spatial(restir_ctx* ctx, const restir_camera* cam, const restir_features* f,
                                   uint32_t rng_key, int debug);
restir_status restir_stage_final(restir_ctx* ctx, const restir_camera* cam, const restir_features* f);

/* R-MIS / R-OMIS stages (render.cpp:64-265) on the stage buffers (the stage region is the whole image):
 *   neighbours     : GBUF -> MIS_NBR (generateResampleIndicesGrid); keys = RESTIR_STAGE_NEIGHBOURS passes 0 and 1
 *   mis_accumulate : iteration i's reservoirs RES_A / RES_B / RES_DBG (restir_stage_ris with debug != 0) + GBUF +
 *                    MIS_NBR -> MIS_ACC (features->ray_trace_mode selects R-MIS or R-OMIS; MIS_ACC is zeroed
 *                    when iteration == 0)
 *   mis_finish     : MIS_ACC -> RGB (combineToScreen, or R-OMIS's per-pixel least-squares solve)
 * restir_stage_mis_capacity: the neighbourhood capacity `cap` of MIS_NBR for these features. */
restir_status restir_stage_neighbours(restir_ctx* ctx, const restir_features* f, uint32_t key_similar,
                                      uint32_t key_dissimilar);
restir_status restir_stage_mis_accumulate(restir_ctx* ctx, const restir_camera* cam, const restir_features* f,
                                          uint32_t iteration);
restir_status restir_stage_mis_finish(restir_ctx* ctx, const restir_features* f);
restir_status restir_stage_mis_capacity(restir_ctx* ctx, const restir_features* f, uint32_t* out_cap);

/* Batched least squares as renderROMIS solves its systems (Eigen CompleteOrthogonalDecomposition::solve,
 * render_utils.h:52): for each of `count` systems x = the minimum-norm least-squares solution of A x = b, A n x n
 * column-major (n*n floats per system), b and x n floats per system; host arrays, n <= RESTIR_ROMIS_MAX_TECHNIQUES.
 * The device routine of the R-OMIS finish, exposed for the parity tests. */
restir_status restir_debug_cod_solve(restir_ctx* ctx, uint32_t n, const float* A, const float* b, float* x,
                                     size_t count);

/* Device portable powf / expf over arrays (parity of the device math with the oracle's). */
restir_status restir_debug_math(restir_ctx* ctx, const float* x, const float* y, float* out_pow, float* out_exp,
                                size_t n);

/* ---- halo-mode frames (multi-GPU tiles with temporal reuse) ----------------------------------------------
 * The stages of restir_render for rank `rank` of a tiles_x x tiles_y split, with the spatial passes' ghost
 * zone replaced by a reservoir exchange (restir_halo_plan).  Per frame:
 *   restir_halo_begin   primary rays on the tile + radius ring, RIS and temporal reuse on the owned tile;
 *                       returns the pack / unpack buffer sizes
 *   per spatial pass:   restir_halo_pack(send) -> move segment i of send to rank send[i].rank and receive
 *                       recv[i] from rank recv[i].rank (RCCL ncclSend/ncclRecv, torch.distributed, ...) ->
 *                       restir_halo_unpack(recv) -> restir_halo_spatial (or the split / native forms below)
 *   restir_halo_end     final shading of the owned tile; *out_next = the grid for the next frame's temporal reuse
 * Bit-identical to the same pixels of a single-GPU restir_render frame.  Buffers are device memory (or host
 * memory when host_memory != 0, staged by the library); pack returns after the buffer is written, unpack
 * expects the received bytes complete when called. */
restir_status restir_halo_begin(restir_ctx* ctx, const restir_camera* cam, const restir_features* features,
                                uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tiles_y, uint32_t rank,
                                const restir_frame* prev, uint64_t* send_bytes, uint64_t* recv_bytes);
/* restir_halo_begin over an uneven layout (restir_tile_layout): rank `rank`'s tile of it */
restir_status restir_halo_begin_layout(restir_ctx* ctx, const restir_camera* cam, const restir_features* features,
                                       const restir_tile_layout* layout, uint32_t rank, const restir_frame* prev,
                                       uint64_t* send_bytes, uint64_t* recv_bytes);
restir_status restir_halo_pack(restir_ctx* ctx, void* send_buf, uint64_t bytes, int host_memory);
restir_status restir_halo_unpack(restir_ctx* ctx, const void* recv_buf, uint64_t bytes, int host_memory);
restir_status restir_halo_spatial(restir_ctx* ctx);
restir_status restir_halo_end(restir_ctx* ctx, restir_frame** out_next, float* out_rgb);

/* A spatial pass in two launches, so that the exchange overlaps computation: the interior of the owned tile
 * (pixels more than `radius` from every side that faces another tile: their neighbourhoods never reach the
 * ring) reads no exchanged reservoir and may run as soon as the pass's pack is issued; the border strips run
 * after the unpack.  Per pass: pack -> spatial_interior -> (exchange) -> unpack -> spatial_border.
 * restir_halo_spatial == spatial_interior + spatial_border.  Same results either way. */
restir_status restir_halo_spatial_interior(restir_ctx* ctx);
restir_status restir_halo_spatial_border(restir_ctx* ctx);

/* Native RCCL transport of the halo (the exchange runs inside the library, no host round trip).  One rank
 * calls restir_rccl_unique_id and hands the RESTIR_RCCL_ID_BYTES bytes to every rank (any side channel);
 * every rank then calls restir_halo_attach_rccl(ctx, id, nranks, rank) once (ncclCommInitRank on the context's
 * device; the communicator lives with the context), or restir_halo_attach_comm with the caller's own
 * ncclComm_t (not owned, it must outlive the context's use).  restir_halo_pass then runs one spatial pass of
 * the frame begun by restir_halo_begin: pack on the context's stream; ncclGroupStart / ncclSend+ncclRecv per
 * plan segment / ncclGroupEnd on the context's communication stream, ordered after the pack by an event; the
 * interior pass on the context's stream concurrently with the transfer; unpack and border pass after it.
 * Nothing synchronises the host.  librccl is loaded on first use (RESTIR_ERR_UNSUPPORTED when absent). */
#define RESTIR_RCCL_ID_BYTES 128u
restir_status restir_rccl_unique_id(void* out, size_t bytes);
restir_status restir_halo_attach_rccl(restir_ctx* ctx, const void* unique_id, uint32_t nranks, uint32_t rank);
restir_status restir_halo_attach_comm(restir_ctx* ctx, void* nccl_comm);
restir_status restir_halo_pass(restir_ctx* ctx);

/* The point-to-point operations restir_halo_pass posts for every spatial pass, in posting order: one ncclSend
 * then one ncclRecv per restir_halo_plan segment, all inside one ncclGroupStart / ncclGroupEnd on the
 * communication stream.  Each: kind, peer (tile rank), byte offset into the pass's device send / receive buffer,
 * bytes, and the global pixel rectangle the bytes hold ([sub-reservoir][pixel row-major][res_a, res_b]).  Pure
 * host: restir_halo_begin builds the list restir_halo_pass posts from with this same function.  *count: in =
 * capacity (2 per segment; 16 suffices), out = operations. */
#define RESTIR_HALO_OP_SEND 0u
#define RESTIR_HALO_OP_RECV 1u
typedef struct restir_halo_op {
    uint32_t kind, peer;
    uint64_t offset, bytes;
    uint32_t x0, y0, width, height;          /* global pixel rectangle */
} restir_halo_op;
restir_status restir_halo_ops(uint32_t global_width, uint32_t global_height, uint32_t tiles_x, uint32_t tiles_y,
                              uint32_t rank, uint32_t radius, uint32_t N, restir_halo_op* ops, uint32_t* count);
restir_status restir_layout_halo_ops(const restir_tile_layout* layout, uint32_t rank, uint32_t radius, uint32_t N,
                                     restir_halo_op* ops, uint32_t* count);

/* Record-only mode of restir_halo_pass: the native transport's plumbing checked without a second GPU.  With
 * restir_halo_record(ctx, 1) a pass needs no communicator and posts no RCCL operation; it appends every step it
 * issues to the context's log instead -- on the context stream (0) the pack launch and the `packed` event, on the
 * communication stream (1) the wait for it, the group with each send / receive (peer, offset, bytes), the `moved`
 * event, then on the context stream the interior launch, the wait for `moved`, the unpack and the border launches
 * -- and otherwise runs the pass with a zeroed receive buffer (the border strips then read zero reservoirs: not a
 * valid image).  restir_halo_log copies the log out in issue order and clears it; *count: in = capacity, out =
 * entries (RESTIR_ERR_INVALID, nothing cleared, when the capacity is short: *count = entries needed).  Attaching a
 * communicator (restir_halo_attach_rccl / _attach_comm) ends record-only mode. */
#define RESTIR_HALO_EV_PACK         0u
#define RESTIR_HALO_EV_RECORD       1u   /* peer: 0 = `packed`, 1 = `moved` */
#define RESTIR_HALO_EV_WAIT         2u   /* peer: the event waited for, as above */
#define RESTIR_HALO_EV_GROUP_START  3u
#define RESTIR_HALO_EV_SEND         4u
#define RESTIR_HALO_EV_RECV         5u
#define RESTIR_HALO_EV_GROUP_END    6u
#define RESTIR_HALO_EV_INTERIOR     7u
#define RESTIR_HALO_EV_UNPACK       8u
#define RESTIR_HALO_EV_BORDER       9u
typedef struct restir_halo_event {
    uint32_t what, stream, peer, pass;
    uint64_t offset, bytes;
} restir_halo_event;
restir_status restir_halo_record(restir_ctx* ctx, int on);
restir_status restir_halo_log(restir_ctx* ctx, restir_halo_event* out, uint32_t* count);

/* ---- frame output (pure host, no device needed) --------------------------------------------------------
 * restir_rgb_to_rgba8: Screen::writeBitmapToFile's conversion (screen.cpp:45-51): glm::clamp(c, 0, 1), then
 * glm::u8vec4(vec4(c, 1) * 255) (truncation toward zero), for `pixels` float RGB triples -> RGBA bytes.
 * restir_encode_bmp / restir_write_bmp: that conversion of a width x height float RGB image (row 0 = top, the
 * layout restir_render returns) written as stbi_write_bmp(path, w, h, 4, data) writes it (screen.cpp:55):
 * BITMAPV4 header, 32 bpp BGRA rows bottom-up.  encode: out == NULL queries *length.
 * restir_features_json: the configuration record renderRayTraced saves per render (render.cpp:281-287,
 * cereal::JSONOutputArchive of struct Features, common.h:138-147), byte for byte; `extra` carries the Features
 * fields the ReSTIR path does not read (NULL: the struct's defaults).  out == NULL queries *length (without the
 * terminating NUL, which is written).  Non-finite gamma / exposure: RESTIR_ERR_INVALID (cereal throws). */
typedef struct restir_features_record_extra {
    uint8_t  enable_recursive;         /* false */
    uint8_t  enable_hard_shadow;       /* true  */
    uint8_t  enable_soft_shadow;       /* true  */
    uint8_t  enable_normal_interp;     /* true  */
    uint8_t  enable_accel_structure;   /* true  */
    uint8_t  reserved[3];
    uint32_t max_reflection_recursion; /* 5 */
} restir_features_record_extra;
restir_status restir_rgb_to_rgba8(const float* rgb, size_t pixels, uint8_t* rgba);
restir_status restir_encode_bmp(const float* rgb, uint32_t width, uint32_t height, uint8_t* out, size_t capacity,
                                size_t* length);
restir_status restir_write_bmp(const char* path, const float* rgb, uint32_t width, uint32_t height);
/* The bytes restir_encode_bmp puts before the pixels of a width x height image (the file and V4 headers): a
 * RESTIR_IMAGE_BGRA8_BOTTOM_UP snapshot appended to them is the BMP file.  out == NULL queries *length. */
restir_status restir_bmp_header(uint32_t width, uint32_t height, uint8_t* out, size_t capacity, size_t* length);
restir_status restir_features_json(const restir_features* features, const restir_features_record_extra* extra,
                                   char* out, size_t capacity, size_t* length);

/* Measured HBM read bandwidth of this device (the roofline's practical ceiling next to the 8 TB/s spec): a
 * streaming-read kernel over `bytes` (rounded down to 16 B; pass >= 1 GiB to defeat the 256 MB Infinity
 * Cache), timed with HIP events over `iters` launches.  *out_gbps = bytes * iters / time / 1e9. */
restir_status restir_measure_read_bandwidth(restir_ctx* ctx, uint64_t bytes, uint32_t iters, double* out_gbps);

/* Background pixels of the last restir_render frame (the compulsory-byte roofline, bench.py roofline.frac_compulsory):
 * the pixels of the RIS tiles (32 x 8 over the frame's computed region) whose every pixel missed the scene with the RIS
 * result known -- the MissTiles flags from which the spatial passes and final shading write those tiles without reading
 * them.  *computed = the region's pixels; *background = 0 when the frame kept no flags (temporal reuse, N > 2, knob
 * "miss.tiles" off).  Synchronises the context's stream. */
restir_status restir_background_pixels(restir_ctx* ctx, uint64_t* background, uint64_t* computed);

/* restir_render frames of this context so far that read the kept G-buffer (tuning "gbuf.reuse") instead of tracing
 * their primary rays; restir_timings counts both kinds under RESTIR_K_PRIMARY_RIS. */
restir_status restir_gbuf_reuses(restir_ctx* ctx, uint64_t* out_frames);

/* restir_render frames of this context so far whose fused last pass took the view's candidate triangle lists (tuning
 * "final.lists") instead of the BVH: from the second consecutive frame that reuses the kept G-buffer with the light list
 * unchanged.  A frame that read its rays' answers from the visibility bits built over those lists (below) counts too. */
restir_status restir_shadow_list_frames(restir_ctx* ctx, uint64_t* out_frames);

/* ... of which those whose last pass read every shadow ray's answer from the view's visibility bits (tuning "final.vis",
 * "final.vis_after"): one bit per (pixel, point light), the lists' rays traced once for a view that stands still.  The
 * bits live exactly as long as the lists they were built over.  restir_shadow_vis_builds: how often they were built. */
restir_status restir_shadow_vis_frames(restir_ctx* ctx, uint64_t* out_frames);
restir_status restir_shadow_vis_builds(restir_ctx* ctx, uint64_t* out_builds);

/* Test hook for those bits, as the last frame left them (RESTIR_ERR_STATE when there are none for the kept G-buffer):
 * for every pixel of that frame's owned rectangle, width x height (RESTIR_ERR_INVALID when the frame's was another size;
 * row-major from its first row, one byte each), the stored answer for point light `light` (< num_lights, else
 * RESTIR_ERR_INVALID: the zero sample has no bits), 1 visible / 0 occluded; 0xFF where none is held -- a pixel of a
 * background tile or one that shows no surface. */
restir_status restir_debug_shadow_vis(restir_ctx* ctx, uint32_t light, uint32_t width, uint32_t height, uint8_t* out_bits);

/* restir_render frames of this context so far whose RIS read its candidates' target pdfs from the view's p-hat table
 * (tuning "ris.phat", "ris.phat_after", "ris.phat_max_mb"): one float per (pixel, point light) of a view that stands still
 * with its lights and materials unchanged -- N = 1, point lights (at most 128), at most 32 candidates, no initial
 * visibility rays, with or without temporal reuse; other shapes run as before.  The first frame after the view, the
 * geometry, the lights or the materials change frees it.  The table takes 4 bytes x the light count (padded to a multiple of 4) per pixel of the view's 32 x 8 tiles: 1,013 MiB for
 * 1920 x 1080 and 128 lights.  A table over ris.phat_max_mb MiB, or one the device has no memory for, is not built and
 * the frames run without it.  restir_phat_builds: how often it was built. */
restir_status restir_phat_frames(restir_ctx* ctx, uint64_t* out_frames);
restir_status restir_phat_builds(restir_ctx* ctx, uint64_t* out_builds);

/* RIS look-ahead (tuning "frames.ahead", "frames.ahead_after", "frames.ahead_prio").  A restir_render frame of a still
 * view whose RIS reads the p-hat table, without temporal reuse, launches the next frame's RIS on a second stream of the
 * context beside its own last pass, into a second set of handle and pdf-cache planes (12 bytes per pixel of the view);
 * the next restir_render call takes that result, and launches no RIS, when everything the result depends on is what the
 * call asks for -- seed, frame index, view, scene, table, features, knobs -- and otherwise runs as if there had been
 * none.  Frames are bit for bit the frames of frames.ahead = 0.  frames.ahead: 0 off, 1 (default) the look-ahead
 * enqueued behind the last pass, 2 before it; frames.ahead_after: from this many consecutive reusing frames (default 4,
 * and never before the table is read); frames.ahead_prio: 1 creates the second stream at the lowest priority.
 * restir_synchronize, restir_timings, scene and light updates and restir_destroy wait for the second stream too; a
 * look-ahead launch is timed as RESTIR_K_PRIMARY_RIS.  A view that moves after a pause pays for one launch that is
 * never read (restir_ahead_discards counts them); restir_set_seed always drops a pending result.
 * From frames.batch_after consecutive reusing frames on (default 8; never effective below frames.ahead_after) a
 * look-ahead launch runs RIS for two frames in one pass over the table (frames.batch: 2, the default; 1 keeps the single
 * launch) and the two calls after take its results in turn, each from a plane set of its own (12 bytes a pixel; three
 * sets beside the frame's own from the first batch on).  A batch is timed as one RESTIR_K_PRIMARY_RIS launch.
 * restir_ahead_discards counts launches with at least one result nobody took.
 * restir_ahead_frames: the frames so far that took their RIS result from a look-ahead. */
restir_status restir_ahead_frames(restir_ctx* ctx, uint64_t* out_frames);
restir_status restir_ahead_discards(restir_ctx* ctx, uint64_t* out_discards);

/* Test hook for that table, as the last frame left it (RESTIR_ERR_STATE when there is none for the kept G-buffer): for
 * every pixel of that frame's view, width x height (RESTIR_ERR_INVALID when the frame's was another size; row-major from
 * its first row), the stored target pdf of point light `light` (< num_lights, else RESTIR_ERR_INVALID); -1 where none is
 * held -- a pixel of a background tile or one that shows no surface. */
restir_status restir_debug_phat(restir_ctx* ctx, uint32_t light, uint32_t width, uint32_t height, float* out_phat);

/* Test hook for those lists, as the last frame left them (RESTIR_ERR_STATE when there are none for the kept G-buffer):
 * for every pixel of that frame's owned rectangle, width x height (RESTIR_ERR_INVALID when the frame's was another
 * size; row-major from its first row, one byte each), the shadow ray from the
 * pixel's hit point to point light `light` (num_lights: the zero sample at the origin) traced by the BVH walk (out_bvh)
 * and over the pixel's tile's list (out_list), 1 visible / 0 occluded; 0xFF in both for a pixel of a background tile. */
restir_status restir_debug_shadow_lists(restir_ctx* ctx, uint32_t light, uint32_t width, uint32_t height, uint8_t* out_bvh,
                                        uint8_t* out_list);

/* What restir_set_scene derived from the scene it uploaded -- the facts the route functions choose kernels by -- so that a
 * test can tell which form a scene took (a light grid the regular form, a BVH past the LDS budget).  Read-only: runs no
 * kernel, changes nothing.  RESTIR_ERR_STATE before the first scene.  (In C++ the function hides the struct's name:
 * write `struct restir_scene_info`.) */
struct restir_scene_info {
    uint32_t num_nodes, num_tris;   /* the flattened BVH (tuning "bvh.max_leaf" at the upload) */
    uint64_t bvh_lds_bytes;         /* (2 num_nodes + 3 num_tris) * 16: staged in LDS while <= 65,536 */
    uint32_t num_lights;
    uint32_t light_types;           /* bit t set <=> a light of restir_light_type t is present */
    uint32_t lights_pgram;          /* every light a parallelogram with one colour at its four corners */
    uint32_t lights_grid;           /* ... that also shares light 0's edges */
    uint32_t lights_regular;        /* ... laid out as regularLightGrid does, ny a power of two */
    uint32_t grid_ny_log2;          /* log2(ny) of a regular grid, else 0 */
    float    light_scale;           /* num_lights when it is a power of two (RIS weights pdf * L), else 0 (pdf / (1 / L)) */
    uint32_t nodes_q_ok;            /* 1: the shadow rays' 16-byte quantized nodes exist (< 65,536 nodes, leaves of < 16
                                     * triangles within the first 4,096); 0: tuning "final.qbvh" falls back to the float nodes */
};
restir_status restir_scene_info(restir_ctx* ctx, struct restir_scene_info* out);

/* ---- timing ----------------------------------------------------------------------------------------- */
/* When enabled, every kernel of restir_render / restir_stage_* is bracketed by HIP events on the
 * context's stream; restir_timings returns the accumulated milliseconds and launch counts per kernel. */
typedef enum restir_kernel {
    RESTIR_K_PRIMARY = 0, RESTIR_K_RIS = 1, RESTIR_K_TEMPORAL = 2, RESTIR_K_SPATIAL = 3, RESTIR_K_FINAL = 4,
    RESTIR_K_PRIMARY_RIS = 5,   /* primary rays + initial RIS fused (restir_render, tuning "fuse.primary_ris") */
    RESTIR_K_MIS = 6,           /* R-MIS / R-OMIS neighbour selection, per-iteration combination, finish */
    RESTIR_K_COUNT = 7
} restir_kernel;
restir_status restir_enable_timing(restir_ctx* ctx, int enable);
/* Launch-shape knobs (never change results): "primary.lds", "ris.lds", "final.lds" (stage the BVH / light table in
 * LDS when it fits), "fuse.primary_ris" (restir_render runs primary rays + RIS as one kernel), "fuse.temporal" (with a predecessor
 * grid, temporal reuse runs inside that kernel: N = 1 / 2, point lights, the light table in LDS; default 1), "spatial.lean" (the
 * lean N = 1 / 2 passes; 0: the general kernels), "timing.mask": the kernels (bit 1 << RESTIR_K_*) restir_enable_timing
 * brackets with HIP events (default all).  "bvh.max_leaf": triangles per BVH leaf for the next restir_set_scene
 * (default 2).  "layout.records": restir_render's buffers as per-pixel records [n_t, res_a, res_b] (1) or SoA planes
 * (0, default).  "ris.compact": initial RIS (N = 1, 2) reads a compact light table when the scene allows one -- point
 * lights only, a light grid, one-colour parallelograms -- instead of the 7-float4 records (default 1; restir_set_scene
 * detects the form bit for bit).  "spatial.xcd_rows|xcd_cols" (the spatial pass's XCD chunk shape; 255 = automatic),
 * "spatial.th" (0: auto, 1: 32x8, 2: 32x16 tiles), "spatial.handles" (N = 1 biased passes over a point-light scene read
 * sample handles, k_spatial1h; with temporal reuse when the predecessor frame carries the handles its last pass wrote
 * -- N = 1 point lights, no ghost ring, the same scene upload -- else its reservoir planes are read; default 1),
 * "spatial.gather" (the point-light handle pass on 32x16 tiles gathers the accepted neighbours' handles instead of
 * staging the handle windows in LDS, k_spatial1hg_t2; default 1), "spatial.n2h" (N = 2 biased passes over a point-light
 * scene without temporal reuse read 16-byte handle records, k_spatial2hg; default 1), "final.qbvh" (final shading's
 * shadow rays walk 16-byte quantized BVH nodes: 0 never, 1 always, 2 = at N = 2, the default), "primary.tl" (the fused
 * primary + RIS kernel's primary rays test their 32x8 tile's candidate triangles -- those not wholly outside the tile's
 * ray pyramid -- instead of walking the BVH; default 1), "ris.late" (stage the light table after the primary rays, only
 * for tiles that need it), "final.sort" (bin each tile's shadow rays by target), "final.fuse" (restir_render shades
 * inside the last N = 1 point-light handle pass, k_spatial1hg_t2_final, where that pass and the binned final kernel would
 * both run -- timed as RESTIR_K_SPATIAL, RESTIR_K_FINAL then has no launches; 0: always two kernels; default 1),
 * "final.miss" (final shading reads only p_mat and
 * (pos, W) for a primary-ray miss), "miss.tiles" (background-tile flags from RIS to the spatial passes and final
 * shading, N <= 2 without temporal reuse), "miss.gbuf" (0 / 1 / 2 = auto: RIS also skips background tiles' G-buffer
 * stores), "gbuf.reuse" (a context keeps the G-buffer and tile flags of the last view restir_render traced -- scene
 * upload, camera, image size, tile -- and a frame of the same view runs the k_gbuf_ris family over them instead of
 * tracing the primary rays again, timed as RESTIR_K_PRIMARY_RIS like the kernel it stands in for; setting any knob, a
 * scene upload, a stage or halo call make the next frame trace; SoA planes only; 0: every frame traces; default 1),
 * "timing.every" / "timing.fence" (event sampling), "mis.chunk" (R-OMIS samples per launch pair).  All default
 * on where measured faster.  Round 5 removed the knobs measured slower in two rounds (persistent *.blocks grids, the
 * RIS work queue, the gather-only spatial pass, non-XCD / row-wave tile orders, 1-D primary / final maps, frames in
 * flight): unknown keys are RESTIR_ERR_INVALID. */
restir_status restir_set_tuning(restir_ctx* ctx, const char* key, int value);
restir_status restir_timings(restir_ctx* ctx, double* ms /*[RESTIR_K_COUNT]*/, uint64_t* launches /*[RESTIR_K_COUNT]*/);
restir_status restir_reset_timings(restir_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* RESTIR_C_H */
