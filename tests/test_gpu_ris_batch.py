"""frames.batch (DESIGN.md §6 "RIS batch"): from the frames.batch_after-th reusing frame of a still view on, one look-ahead
launch (k_gbuf_ris_n1_lds_pt_phat_batch2) runs RIS for two frames in one pass over the p-hat table, and the two frames
after take its results in turn.  Each key's candidate loop is the one-key kernel's under that key, so every frame must
equal, bit for bit, the frame of a context with frames.ahead = 0 -- no tolerances anywhere in this file.

Frame numbers as in test_gpu_ris_ahead.py (its helpers are used): frame 0 traces, frame k >= 1 is the k-th reusing frame.
Both contexts run ris.phat_after = frames.ahead_after = frames.batch_after = AFTER = 3, so frame 3 builds the table, runs
its own RIS and launches the first batch (frames 4 and 5); ahead_frames() reads max(0, k - AFTER) after frame k.

The two cadences (frames.batch_form): 0 launches a batch when no result waits -- beside frames 3, 5, 7, ...; 1 launches when
at most one waits -- beside frames 3, 4, 6, 8, ..., so that after an even frame the results of two launches wait (three
results) and after an odd one the two results of one launch.  ahead_discards() counts launches with a result nobody
took: a change made while one batch's results wait (either or both) adds exactly 1; under form 1 a change after an even
frame finds two launches waiting and adds 2 -- that is what the counter means, and the case is asserted as such.
"""
import pytest

from romis_amd import scene
from test_gpu_parity import SEED, assert_bits, get_scene
from test_gpu_phat_table import mixed_materials
from test_gpu_ris_ahead import AFTER, SIZES, Pair, features, pair  # noqa: F401  (pair: the fixture)
from test_gpu_shadow_lists import NIGHTCLUB, camera, lights_around, make_scene, point_light

pytestmark = pytest.mark.gpu

FORMS = [0, 1]


def batch_pair(pair, sc, **knobs):
    knobs.setdefault("frames__batch_after", AFTER)
    return pair(sc, **knobs)


def launches_after(frames, form, batch=2):
    """RIS launches of frames 0 .. frames - 1 of a still view (the header's ris_batch_launch, restated): every frame up to
    AFTER runs its own; from frame AFTER on a look-ahead launch whenever few enough results wait"""
    n, pending = 0, 0
    for k in range(frames):
        if k <= AFTER:
            n += 1
        else:
            pending -= 1
        if k >= AFTER:
            if batch == 2 and pending <= form:
                n, pending = n + 1, pending + 2
            elif batch == 1 and pending == 0:
                n, pending = n + 1, pending + 1
    return n


def run_frames(p, cam, w, h, f, what, n=11, form=1, timed=4, **kw):
    """Frames 0 .. n - 1 of a still view on both contexts, the counters checked after each; then `timed` more with every
    launch timed (the timing knobs keep the pending results), whose RIS launch count is the cadence's: that the frames
    are equal is then known to be the batch kernel's doing -- single launches would count one a frame"""
    for frame in range(n):
        p.frame(cam, w, h, f, what, **kw)
        assert p.new.ahead_frames() == max(0, frame - AFTER), f"{what}: frame {frame}"
        assert p.new.ahead_discards() == 0, f"{what}: frame {frame}"
    if not timed:
        return
    p.new.set_tuning("timing.mask", -1)
    p.new.set_tuning("timing.every", 1)
    p.new.reset_timings()
    p.new.enable_timing(True)
    for frame in range(n, n + timed):
        p.frame(cam, w, h, f, what, **kw)
        assert p.new.ahead_frames() == frame - AFTER and p.new.ahead_discards() == 0, f"{what}: frame {frame}"
    p.new.synchronize()
    p.new.enable_timing(False)
    kt = p.new.timings()
    want = launches_after(n + timed, form) - launches_after(n, form)
    assert want < timed and kt["primary_ris"][1] == want and kt["spatial"][1] == timed * f.spatial_resampling_passes, what


# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", [NIGHTCLUB, "cube_points"])
def test_still_frames_equal_and_counted(pair, name, w, h):
    """11 frames: the run ends on a batch's first result under form 1 and on its second under form 0"""
    p = batch_pair(pair, make_scene(name))
    run_frames(p, camera(name, w, h), w, h, features(1), f"{name} {w}x{h}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [10, 11])
def test_both_forms_and_both_ends(pair, form, n):
    w, h = 70, 37
    p = batch_pair(pair, make_scene(NIGHTCLUB), frames__batch_form=form)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), f"form {form}, {n} frames", n=n, form=form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", [16, 5, 1])
def test_candidate_counts(pair, M, form):
    """Ragged chunks (5 over four lanes) and lanes without a candidate (1)"""
    w, h = 70, 37
    p = batch_pair(pair, make_scene(NIGHTCLUB), frames__batch_form=form)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1, M=M), f"M = {M}", form=form)


def test_33_lights(pair):
    """A light count that is no multiple of 4 (row padding, a non-power-of-two uniform_index), mixed materials"""
    w, h = 70, 37
    base = get_scene(NIGHTCLUB)
    sc = scene.Scene(mixed_materials(base), lights_around(base, 32, 44, radius=0.3), "nightclub_mixed_33pt")
    assert len(sc.lights) == 33
    p = batch_pair(pair, sc)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), "33 lights")


@pytest.mark.parametrize("form", FORMS)
def test_two_passes(pair, form):
    w, h = 70, 37
    p = batch_pair(pair, make_scene(NIGHTCLUB), frames__batch_form=form)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(2), "two passes", form=form)


@pytest.mark.parametrize("w,h", SIZES[:2])
def test_ghost_ring_tile(pair, w, h):
    from romis_amd import restir
    p = batch_pair(pair, make_scene(NIGHTCLUB))
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    tile = restir.tile_plan(w, h, 2, 1, 1, f.spatial_resample_radius)
    assert tile.x0 > 0 and tile.gx0 > 0
    run_frames(p, cam, w, h, f, f"tile {w}x{h}", tile=tile)


@pytest.mark.parametrize("form", FORMS)
def test_images_left_on_the_device(pair, form):
    w, h = 70, 37
    p = batch_pair(pair, make_scene(NIGHTCLUB), frames__batch_form=form)
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), "device image", form=form, want_grid=False, want_rgb=False)


def test_batch_1_equals_the_default(pair):
    """frames.batch = 1 (single launches throughout) against the default, which batches: bit for bit, frame by frame"""
    w, h = 70, 37
    sc = make_scene(NIGHTCLUB)
    one, two = batch_pair(pair, sc, frames__batch=1), batch_pair(pair, sc)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    for frame in range(11):
        a, _ = one.new.render_restir(None, cam, w, h, f, want_grid=False)
        b, _ = two.new.render_restir(None, cam, w, h, f, want_grid=False)
        assert_bits(a, b, f"frame {frame}: frames.batch=1 against the default")
        assert one.new.ahead_frames() == two.new.ahead_frames() == max(0, frame - AFTER)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("batch", [1, 2])
def test_timings_count_a_batch_as_one_launch(pair, form, batch):
    w, h = 70, 37
    p = batch_pair(pair, make_scene(NIGHTCLUB), frames__batch_form=form, frames__batch=batch)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    p.new.set_tuning("timing.mask", -1)
    p.new.set_tuning("timing.every", 1)
    p.new.enable_timing(True)
    for frame in range(11):
        p.frame(cam, w, h, f, "timed", want_grid=False)
    p.new.synchronize()
    kt = p.new.timings()
    assert kt["primary_ris"][1] == launches_after(11, form, batch) and kt["spatial"][1] == 11
    assert p.new.ahead_frames() == 10 - AFTER and p.new.ahead_discards() == 0


# --------------------------------------------------------------------------------------------------------
# invalidation in the middle of a batch.  `frames` frames first: AFTER + 1 leaves the first batch's two results waiting;
# AFTER + 2 leaves its second (under form 1 beside the next batch's two)
def change(p, kind, sc, w, h):
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    if kind == "camera":
        cam = scene.make_camera(30.0, 60.0, (2.57, 1.23, -1.35), (10.3, 30.0, 0.0), w, h)
    elif kind == "seed":
        p.each(lambda r: r.set_seed(SEED + 1, 6))
    elif kind == "M":
        f = features(1, M=16)
    elif kind == "lights":
        moved = [point_light([l.p0[0] + 0.25, l.p0[1], l.p0[2] - 0.5], list(l.c0)) for l in sc.lights]
        p.each(lambda r: r.set_lights(moved))
    return cam, f


@pytest.mark.parametrize("kind", ["camera", "seed", "M", "lights"])
@pytest.mark.parametrize("form,frames,discards", [(0, AFTER + 1, 1), (0, AFTER + 2, 1), (1, AFTER + 1, 1), (1, AFTER + 2, 2)])
def test_change_in_the_middle_of_a_batch(pair, kind, form, frames, discards):
    w, h = 70, 37
    sc = make_scene(NIGHTCLUB)
    p = batch_pair(pair, sc, frames__batch_form=form)
    what = f"{kind}, form {form}, after {frames} frames"
    run_frames(p, camera(NIGHTCLUB, w, h), w, h, features(1), what, n=frames, timed=0)
    before = p.new.ahead_frames()
    cam, f = change(p, kind, sc, w, h)
    p.frame(cam, w, h, f, what)   # equals frames.ahead = 0's
    assert p.new.ahead_discards() == discards, what
    assert p.new.ahead_frames() == before, f"{what}: a stale result was taken"
    for _ in range(8):
        p.frame(cam, w, h, f, what)
    assert p.new.ahead_discards() == discards, what
    assert p.new.ahead_frames() >= before + 4, f"{what}: the batch did not re-engage"


@pytest.mark.parametrize("form", FORMS)
def test_close_and_set_scene_with_a_batch_in_flight(pair, form):
    w, h = 96, 48
    sc = make_scene(NIGHTCLUB)
    cam, f = camera(NIGHTCLUB, w, h), features(1)
    p = batch_pair(pair, sc, frames__batch_form=form)
    run_frames(p, cam, w, h, f, "first", n=AFTER, timed=0)
    p.new.render_restir(None, cam, w, h, f, want_grid=False, want_rgb=False)   # launches the first batch; nothing waits
    p.new.close()
    from romis_amd import restir
    p.new = restir.Renderer(0)
    for k in ("ris.phat_after", "frames.ahead_after", "frames.batch_after"):
        p.new.set_tuning(k, AFTER)
    p.new.set_tuning("frames.batch_form", form)
    p.new.set_scene(sc)
    p.new.set_seed(SEED, 0)
    p.old.set_seed(SEED, 0)
    for _ in range(AFTER):
        p.frame(cam, w, h, f, "after close")
    p.new.render_restir(None, cam, w, h, f, want_grid=False, want_rgb=False)
    p.old.render_restir(None, cam, w, h, f, want_grid=False, want_rgb=False)
    p.each(lambda r: r.set_scene(make_scene("cube_points")))
    assert p.new.ahead_discards() == 1 and p.new.ahead_frames() == 0
    cube = camera("cube_points", w, h)
    for _ in range(AFTER + 3):
        p.frame(cube, w, h, f, "after set_scene")
    assert p.new.ahead_frames() == 2 and p.new.ahead_discards() == 1
