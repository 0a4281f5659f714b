"""The input rows of tests/golden/launch_routes.txt (row format: tests/cpp/route_rows.h), one per line on stdout.

    python scripts/launch_route_matrix.py > rows.txt

The matrix takes the full product of features (N, K, R, biased / unbiased, spatial_vis) with the scene and ask classes a
stage reads, walks the regions and flips the knobs one at a time; it is thinned where rows cannot differ (the header of
the golden file says how).
"""
import itertools

DBG, HIN, HOUT, HRD, RPI, RPN, RPO, VIS, MTF, FIN, FRD, NT2, THW = (1 << i for i in range(13))

# num_lights, light_types, grid, pgram, regular
SCENES = {
    "pt32": (32, 1, 0, 0, 0), "pt254": (254, 1, 0, 0, 0), "pt255": (255, 1, 0, 0, 0), "pt4096": (4096, 1, 0, 0, 0),
    "reg1024": (1024, 4, 1, 1, 1), "reg2048": (2048, 4, 1, 1, 1), "grid": (64, 4, 1, 1, 0), "pgram": (64, 4, 0, 1, 0),
    "mixed": (40, 5, 0, 0, 0), "none": (0, 0, 0, 0, 0),
}
# num_nodes, num_tris: 12.5 KB; 255 bytes short of the 64 KB budget (no light table fits beside it); 125 KB
BVHS = {"fit": (100, 200), "tight": (1020, 680), "big": (4000, 3000)}
FEATURES = list(itertools.product((1, 2, 3), (5, 6), (10, 11), (0, 1), (0, 1)))   # N K R unbiased spatial_vis


def region(vw, vh, rw=None, rh=None, records_n=0):
    rw, rh = (vw if rw is None else rw), (vh if rh is None else rh)
    return (vw, vh, rw, rh, 1 + 2 * records_n, 2) if records_n else (vw, vh, rw, rh, 1, vw * vh)


def regions(n):
    return [region(64, 64, 0, 5), region(33, 9), region(767, 64), region(768, 64), region(1920, 1080),
            region(2047, 64), region(2048, 64), region(3840, 2160), region(4097, 16), region(1920, 1080, records_n=n),
            region(20000, 20000, 64, 64),      # 16-byte plane offsets pass 2^32
            region(16384, 12288, 64, 64)]      # ... only with the second sub-reservoir plane (N = 2)


HD = region(1920, 1080)
SEEN = set()
KNOBS = ["spatial.lean:0", "spatial.th:1", "spatial.th:2", "spatial.gather:0", "spatial.handles:0", "spatial.n2h:0",
         "ris.compact:0", "ris.compact:2", "ris.lds:0", "primary.lds:0", "final.sort:0", "final.lds:0", "final.qbvh:0",
         "final.qbvh:1", "final.fuse:0", "final.miss:0", "fuse.temporal:0", "xcd:2:0", "xcd:4:15"]


def row(stage, scene="pt32", bvh="fit", q=1, f=(1, 5, 10, 0, 0), rg=HD, ask=0, mt=(0, 0, 0), passes=1, m0=0, knob="-",
        msz=1, M=32):
    s, b = SCENES[scene], BVHS[bvh]
    key = (stage, s, msz, b, q, tuple(f), M, tuple(rg), ask, tuple(mt), passes, m0, knob)
    if key in SEEN:
        return
    SEEN.add(key)
    groups = [s + (msz,), b + (q,), tuple(f) + (M,), tuple(rg), None, tuple(mt), (passes, m0)]
    defaults = [SCENES["pt32"] + (1,), BVHS["fit"] + (1,), (1, 5, 10, 0, 0, 32), HD, None, (0, 0, 0), (1, 0)]
    words = ["-" if g == d else ",".join(map(str, g)) for g, d in zip(groups, defaults)]
    words[4] = "%x" % ask if ask else "-"
    print(" ".join([stage] + words + [knob]))


def main():
    n12 = (1, 2)
    # primary rays: the regions, then the BVH sizes with and without primary.lds
    for rg in regions(1):
        row("primary", rg=rg, ask=NT2)
    for bvh in BVHS:
        for knob in ("-", "primary.lds:0"):
            row("primary", bvh=bvh, knob=knob)
    # RIS: every light table x N; its knobs where the table has a compact form (N = 1, 2) and ris.lds at every N
    for scene in SCENES:
        for n in (1, 2, 3):
            row("ris", scene=scene, f=(n, 5, 10, 0, 0), ask=DBG | RPO)
            row("ris", scene=scene, f=(n, 5, 10, 0, 0), knob="ris.lds:0")
        for n in n12:
            for knob in ("ris.compact:0", "ris.compact:2"):
                row("ris", scene=scene, f=(n, 5, 10, 0, 0), ask=RPO, knob=knob)
    for rg in regions(1):
        row("ris", rg=rg, ask=RPO)
    # fused primary + RIS: light tables x N with nothing and with everything asked; the BVH sizes; the knobs
    everything = HOUT | HRD | MTF | RPO | NT2 | DBG
    for scene in SCENES:
        for n in (1, 2, 3):
            row("pris", scene=scene, f=(n, 5, 10, 0, 0), rg=region(33, 9))
            row("pris", scene=scene, f=(n, 5, 10, 0, 0), rg=region(33, 9), ask=everything, mt=(0, 0, 3))
        row("pris", scene=scene, bvh="tight", rg=region(33, 9), ask=everything, mt=(0, 0, 1))
        for knob in ("ris.compact:0", "ris.compact:2", "ris.lds:0"):
            row("pris", scene=scene, rg=region(33, 9), ask=everything, mt=(0, 0, 3), knob=knob)
        row("pris", scene=scene, f=(2, 5, 10, 0, 0), rg=region(33, 9), ask=everything, mt=(0, 0, 3), knob="ris.lds:0")
    for n in (1, 2, 3):
        row("pris", bvh="big", f=(n, 5, 10, 0, 0), rg=region(33, 9), ask=everything)
        for scene in ("pt32", "reg1024", "grid", "none"):
            row("pris", scene=scene, f=(n, 5, 10, 0, 0), rg=region(33, 9), ask=MTF, mt=(0, 0, 3))
            row("pris", scene=scene, f=(n, 5, 10, 0, 0), rg=region(33, 9), ask=HOUT | RPO)
    for knob in ("ris.late:0", "primary.tl:0"):
        row("pris", rg=region(33, 9), knob=knob)
    for rg in regions(1) + [region(1920, 1080, records_n=2), region(1920, 1080, records_n=3)]:
        row("pris", f=(1 if rg[4] < 5 else (rg[4] - 1) // 2, 5, 10, 0, 0), rg=rg, ask=MTF | HOUT, mt=(0, 0, 3))
    # ... with temporal reuse
    for scene in SCENES:
        for n in (1, 2, 3):
            row("prist", scene=scene, f=(n, 5, 10, 0, 0), rg=region(33, 9), ask=HOUT | HRD | THW | RPO | NT2)
    for n in (1, 2, 3):
        row("prist", f=(n, 5, 10, 0, 0), rg=region(33, 9))
    for scene in ("pt32", "pt254", "pt4096"):
        for n in n12:
            row("prist", scene=scene, bvh="tight", f=(n, 5, 10, 0, 0), rg=region(33, 9), ask=HOUT | THW)
    row("prist", bvh="big", rg=region(33, 9), ask=HOUT | THW)
    for knob in ("fuse.temporal:0", "ris.compact:0", "ris.lds:0", "ris.late:0"):
        for n in n12:
            row("prist", f=(n, 5, 10, 0, 0), rg=region(33, 9), ask=HOUT | THW, knob=knob)
    for rg in regions(1):
        row("prist", rg=rg, ask=HOUT | THW)
    # spatial passes.  Features in full over point lights: inside the lean kernels' domain every ask set, outside it
    # (K = 6; biased R = 11; N = 3: the general kernels, which take no optional buffer) three
    flags = (32, 1, 0)
    none, cache, vis = (0, (0, 0, 0)), (RPI | RPO | MTF, flags), (VIS | MTF, (32, 0, 0))
    hin, passes_h, last_h = (HIN | RPI, (0, 0, 0)), (HIN | HOUT | HRD | RPI | RPO | MTF, flags), (HIN | HOUT | FIN | RPI | MTF, flags)
    sp_asks = [none, (RPI | RPN | RPO, (0, 0, 0)), cache, vis, hin, passes_h, last_h, (HIN | FIN | DBG, (0, 0, 0))]
    for f in FEATURES:
        n, k, r, ub, sv = f
        if sv and not ub:
            continue   # (a biased pass does not read spatial_vis)
        lean = n != 3 and k == 5 and (ub or r == 10)
        for ask, mt in (sp_asks if lean else (none, cache, passes_h)):
            row("spatial", f=f, ask=ask, mt=mt)
        if lean and not ub:   # a light grid: the handle asks
            for ask, mt in (hin, passes_h, (HIN | DBG, (0, 0, 0))):
                row("spatial", scene="reg1024", f=f, ask=ask, mt=mt)
        if ub and sv:   # shadow rays in the pass: the BVH past the LDS budget
            row("spatial", bvh="big", f=f, ask=vis[0], mt=vis[1])
    for ask, mt in ((DBG, (0, 0, 0)), (HIN | FIN | FRD | RPI, (0, 0, 0)), (HIN | FIN | RPO, (0, 0, 0)), (FIN, (0, 0, 0))):
        row("spatial", ask=ask, mt=mt)
    row("spatial", f=(2, 5, 10, 0, 0), ask=DBG)
    for n in n12:
        for rg in regions(n):
            row("spatial", f=(n, 5, 10, 1, 0), rg=rg)
            for ask, mt in (none, passes_h):
                row("spatial", f=(n, 5, 10, 0, 0), rg=rg, ask=ask, mt=mt)
    for rg in regions(1):
        row("spatial", scene="reg1024", rg=rg, ask=passes_h[0], mt=flags)
    for knob in KNOBS:
        for ask, mt in (none, passes_h, last_h, (DBG, (0, 0, 0)), (HIN | DBG, (0, 0, 0))):   # (the _dbg twins too)
            row("spatial", ask=ask, mt=mt, knob=knob)
        for ask, mt in (passes_h, (HIN | DBG, (0, 0, 0))):
            row("spatial", f=(2, 5, 10, 0, 0), ask=ask, mt=mt, knob=knob)
            row("spatial", scene="reg1024", ask=ask, mt=mt, knob=knob)
        row("spatial", f=(1, 5, 10, 1, 1), ask=VIS, knob=knob)
    for knob in ("spatial.lean:0", "spatial.th:1", "spatial.th:2", "spatial.gather:0", "xcd:2:0", "xcd:4:15"):   # shape knobs
        for scene, n in (("pt32", 1), ("pt32", 2), ("reg1024", 1)):
            for ask, mt in (none, passes_h):
                row("spatial", scene=scene, f=(n, 5, 10, 0, 0), rg=region(2048, 64), ask=ask, mt=mt, knob=knob)
    for scene in SCENES:
        for n in n12:
            row("spatial", scene=scene, f=(n, 5, 10, 0, 0), ask=last_h[0], mt=flags)
    for bvh in BVHS:   # the fused final's LDS bound and node form
        for q in (0, 1):
            for knob in ("-", "final.qbvh:0", "final.qbvh:1", "final.miss:0"):
                row("spatial", bvh=bvh, q=q, ask=last_h[0], mt=flags, knob=knob)
    row("spatial", scene="pt254", bvh="tight", ask=last_h[0], mt=flags)
    # final shading
    for n in (1, 2, 3):
        for bvh in ("fit", "big"):
            for q in (0, 1):
                for knob in ("-", "final.sort:0", "final.lds:0", "final.qbvh:0", "final.qbvh:1", "final.miss:0"):
                    row("final", bvh=bvh, q=q, f=(n, 5, 10, 0, 0), ask=VIS | MTF, knob=knob)
        for ask in (0, VIS, MTF):
            row("final", f=(n, 5, 10, 0, 0), ask=ask)
        row("final", bvh="tight", f=(n, 5, 10, 0, 0), ask=MTF)
        row("final", f=(n, 5, 10, 0, 0), ask=MTF, msz=0)
    for rg in regions(1):
        row("final", rg=rg, ask=MTF)
    # the frame-level predicates
    for f in FEATURES:
        if f[3] or not f[4]:
            for scene, bvh in (("pt32", "fit"), ("pt32", "big"), ("reg1024", "fit")):
                row("pred", scene=scene, bvh=bvh, f=f)
    for scene in SCENES:
        for n in n12:
            row("pred", scene=scene, f=(n, 5, 10, 0, 0))
        row("pred", scene=scene, bvh="tight")
    for knob in KNOBS:
        for n, ub in ((1, 0), (2, 0), (1, 1)):
            row("pred", f=(n, 5, 10, ub, 1), knob=knob)
        row("pred", scene="reg1024", knob=knob)
    for knob in ("fuse.temporal:0", "ris.compact:0", "ris.compact:2", "ris.lds:0"):
        for scene in ("pt254", "pt4096", "grid", "mixed", "none"):
            row("pred", scene=scene, knob=knob)
    # the handle field's M bound, M (K + 1)^passes <= 2^24 - 1 (point lights) or 2^19 - 1 (a light grid): the last M
    # inside and the first outside at one and two passes
    for scene, n in (("pt32", 1), ("pt32", 2), ("reg1024", 1)):
        for passes in (1, 2):
            for M in (14563, 14564, 87381, 87382, 466033, 466034, 2796202, 2796203):
                row("pred", scene=scene, f=(n, 5, 10, 0, 0), passes=passes, M=M)
        row("pred", scene=scene, f=(n, 5, 10, 0, 0), passes=0)
        for m0 in (87381, 87382, 2796202, 2796203, 1 << 33):
            row("pred", scene=scene, f=(n, 5, 10, 0, 0), m0=m0)
    for n in n12:
        for rg in regions(n):
            row("pred", f=(n, 5, 10, 0, 0), rg=rg)


if __name__ == "__main__":
    main()
