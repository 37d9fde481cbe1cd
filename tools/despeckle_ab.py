"""What the despeckle pass does to the rare bright samples of C2 and C3 (include/jade_bvh.h, "Despeckle, stated"), what DESIGN.md 3.23 and 7 quote.

usage: python tools/despeckle_ab.py [--out profiles/despeckle_ab.json] [--scenes C2,C3] [--spps 16,64,256] [--frames 16] [--ref-spp 8192]
                                    [--sweep-spp 64] [--sweep-frames 16] [--no-sweep] [--bench-parent FILE --bench-this FILE]
       python tools/despeckle_ab.py --profile-run     (the program of the rocprofv3 --kernel-trace --stats run: see the end of this text)
           On tools/branch_ab.py's protocol: C2 at 512 x 512 and C3 at 1080p under the reference estimator, --frames frames at each of
           --spps samples from the seeds frame = 1000 k, against ONE frame of --ref-spp samples from the seed frame = 2^20 (DESIGN.md 3.5,
           3.6).  Per scene and sample count, the mean over the frames of four figures
             relMSE              mean over pixel channels of (x - ref)^2 / (ref^2 + 1e-4)
             median_rel_sq_err   the median over pixel channels of the same quantity
             outliers            pixel channels above 8 x (ref + 0.05) - branch_ab.py's rule - summed over the frames
             energy              the frame's mean radiance over the reference's: what the pass removes, its bias
           each for the frame raw, despeckled (jade_despeckle_image on the resolve and jade_render_guides' variance, the shipped
           defaults), denoised (jade_denoise_image, defaults) and despeckled-then-denoised (the despeckled colour AND variance filtered),
           with the report's counts.
           The sweep: at --sweep-spp samples, over the first --sweep-frames of those frames, sigmas in {1, 2, 3, 4, no variance} x gain in
           {1, 1.5, 2, 4} x rank in {1, 2, 3} x radius in {1, 2} x iterations in {1, 2}: relMSE, outliers and energy of the despeckled frame.
           --bench-parent / --bench-this: files of bench.py result lines (bench.py --gpus 1 --steps 4 --warmup 1 with JADE_HIP_LIB on the
           parent's libjade_hip.so, and with this build's, alternating); they go under "bench".
           No threshold: the figures are reported as measured.  A non-parity, opt-in pass, nobody's default.
           --profile-run: one C3 1080p render of 64 samples, then jade_render_despeckle at radius 2 with the default denoise parameters,
           twice (the first call allocates); under rocprofv3 --kernel-trace --stats its k_despeckle<2> line stands beside k_atrous's.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

SIZES = {"C2": (512, 512)}
REL_FLOOR = 1e-4
REF_FRAME = 1 << 20
SWEEP = dict(sigmas=(1.0, 2.0, 3.0, 4.0, None), gain=(1.0, 1.5, 2.0, 4.0), rank=(1, 2, 3), radius=(1, 2), iterations=(1, 2))
VARIANTS = ("raw", "despeckled", "denoised", "despeckled_denoised")


def scene_of(name):
    hs, cfg = J.build_config(name)

    def make(spp, frame=0):
        p = B.params_from_config(cfg)
        if name in SIZES:
            p.width, p.height = SIZES[name]
        p.spp, p.frame, p.walk = spp, frame, _abi.WALK_EARLY_EXIT
        return p
    return hs, make


def render_steps(sc, p, chunk=1024):
    """a frame of p.spp samples in steps of at most `chunk` (a multiple of 1024 above it, so that the variance can be estimated)"""
    sc.begin(p)
    left = p.spp
    while left > 0:
        n = min(left, chunk)
        sc.step(n)
        left -= n


def figures(x, ref, bar, full=True):
    x = x.astype(np.float64)
    r = (x - ref) ** 2 / (ref ** 2 + REL_FLOOR)
    out = dict(relMSE=float(r.mean()), outliers=int((x > bar).sum()), energy=float(x.mean() / ref.mean()))
    if full:
        out["median_rel_sq_err"] = float(np.median(r))
    return out


def mean_rows(rows):
    out = {}
    for k in rows[0]:
        vals = [r[k] for r in rows]
        out[k] = int(sum(vals)) if k == "outliers" or k.startswith("n_") else float(np.mean(vals))
    out["relMSE_per_frame_min_max"] = [float(min(r["relMSE"] for r in rows)), float(max(r["relMSE"] for r in rows))]
    return out


def params(hip, sigmas=None, gain=None, rank=None, radius=None, iterations=None):
    p = hip.despeckle_defaults()
    for k, v in (("sigmas", sigmas), ("gain", gain), ("rank", rank), ("radius", radius), ("iterations", iterations)):
        if v is not None:
            setattr(p, k, v)
    return p


def profile_run():
    hip = J.hip()
    hs, make = scene_of("C3")
    dp = params(hip, radius=2)
    with hip.scene(hs) as sc:
        render_steps(sc, make(64, frame=1000))
        for _ in range(2):
            _, _, _, rep = sc.despeckle(dp, denoise=hip.denoise_defaults(), want_bgr8=False)
    print("profile run: C3 1080p, 64 spp, radius 2 + denoise:", rep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despeckle_ab.json"))
    ap.add_argument("--scenes", default="C2,C3")
    ap.add_argument("--spps", default="16,64,256")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--sweep-spp", type=int, default=64)
    ap.add_argument("--sweep-frames", type=int, default=16)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    if a.profile_run:
        return profile_run()
    hip = J.hip()
    spps = [int(s) for s in a.spps.split(",")]
    d0 = hip.despeckle_defaults()
    res = {"what": __doc__.strip().splitlines()[0], "frames": a.frames, "ref_spp": a.ref_spp, "ref_frame": REF_FRAME, "sweep_spp": a.sweep_spp,
           "sweep_frames": 0 if a.no_sweep else a.sweep_frames,
           "defaults": {k: getattr(d0, k) for k in ("iterations", "radius", "rank", "gain", "floor", "sigmas")}, "scenes": {}}
    if os.path.exists(a.out):  # (the bench runs of parent against this build are kept)
        with open(a.out) as f:
            old = json.load(f)
        if "bench" in old:
            res["bench"] = old["bench"]
    if a.bench_parent and a.bench_this:
        runs = {}
        for key, path in (("parent", a.bench_parent), ("this_build", a.bench_this)):
            with open(path) as f:
                lines = [json.loads(ln) for ln in f if ln.startswith("{")]
            runs[key] = [dict(Mray_per_s=b["value"], ms_per_step=b.get("ms_per_step"), frame_sha256=b["frame_sha256"], rays=b["rays"]) for b in lines]
        res["bench"] = dict(what="bench.py --gpus 1 --steps 4 --warmup 1 (C3, 1024 spp per step) with the parent's libjade_hip.so (JADE_HIP_LIB) and with this build's, "
                                 "alternating in one call on one MI355X", **runs,
                            frame_sha256_equal_in_all_runs=len({r["frame_sha256"] for v in runs.values() for r in v}) == 1)
    dn = hip.denoise_defaults()
    for name in a.scenes.split(","):
        t0 = time.time()
        hs, make = scene_of(name)
        p0 = make(1)
        e = {"width": int(p0.width), "height": int(p0.height), "spp": {}}
        with hip.scene(hs) as sc:
            render_steps(sc, make(a.ref_spp, frame=REF_FRAME))
            ref = sc.resolve(want_bgr8=False)[0].astype(np.float64)
            bar = 8 * (ref + 0.05)
            kept = []  # the sweep's frames: (rgb, variance)
            for spp in spps:
                rows = {v: [] for v in VARIANTS}
                for k in range(1, a.frames + 1):
                    render_steps(sc, make(spp, frame=1000 * k))
                    rgb = sc.resolve(want_bgr8=False)[0]
                    g = sc.guides(dn.guide_spp)
                    ds_rgb, ds_var, _, rep = hip.despeckle_image(rgb, g["variance"])
                    rows["raw"].append(figures(rgb, ref, bar))
                    rows["despeckled"].append(dict(figures(ds_rgb, ref, bar), **rep))
                    rows["denoised"].append(figures(hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], dn), ref, bar))
                    rows["despeckled_denoised"].append(figures(hip.denoise_image(ds_rgb, ds_var, g["albedo"], g["normal"], g["depth"], dn), ref, bar))
                    if spp == a.sweep_spp and k <= a.sweep_frames and not a.no_sweep:
                        kept.append((rgb, g["variance"]))
                e["spp"][str(spp)] = {v: mean_rows(r) for v, r in rows.items()}
                m = e["spp"][str(spp)]
                print(f"{name} {spp} spp: relMSE raw {m['raw']['relMSE']:.4g} despeckled {m['despeckled']['relMSE']:.4g} denoised {m['denoised']['relMSE']:.4g} "
                      f"both {m['despeckled_denoised']['relMSE']:.4g}; outliers {m['raw']['outliers']} -> {m['despeckled']['outliers']}; energy "
                      f"{m['raw']['energy']:.4f} -> {m['despeckled']['energy']:.4f}; clamped {m['despeckled']['n_clamped']} established "
                      f"{m['despeckled']['n_established']}", flush=True)
        if kept:
            sweep = []
            for z, gain, rank, radius, its in itertools.product(*(SWEEP[k] for k in ("sigmas", "gain", "rank", "radius", "iterations"))):
                dp = params(hip, z, gain, rank, radius, its)
                rs = []
                for rgb, var in kept:
                    out, _, _, rep = hip.despeckle_image(rgb, var if z is not None else None, dp)
                    rs.append(dict(figures(out, ref, bar, full=False), **rep))
                row = mean_rows(rs)
                row.pop("n_usable", None)
                sweep.append(dict(sigmas=z, gain=gain, rank=rank, radius=radius, iterations=its, **row))
            e["sweep"] = sweep
            raw = e["spp"][str(a.sweep_spp)]["raw"]
            best = sorted(sweep, key=lambda r: r["relMSE"])[:5]
            print(f"{name} sweep at {a.sweep_spp} spp over {len(kept)} frames (raw relMSE {raw['relMSE']:.4g}); lowest relMSE:")
            for r in best:
                print("   ", {k: r[k] for k in ("sigmas", "gain", "rank", "radius", "iterations", "relMSE", "outliers", "energy")}, flush=True)
        e["seconds"] = time.time() - t0
        res["scenes"][name] = e
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
