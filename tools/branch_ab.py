"""What sharing out the branch draws changes (include/jade_bvh.h: jade_scene_set_branch_sampling): JADE_BRANCH_STRATIFIED against JADE_BRANCH_RANDOM, what DESIGN.md 3.18 and 7 quote.

usage: python tools/branch_ab.py [--out profiles/branch_ab.json] [--scenes C2,C3] [--spp 64] [--frames 16] [--repeats 3] [--ref-spp 4096]
                                 [--bench-parent FILE --bench-this FILE]
           On tools/passes_ab.py's protocol, so that the figures sit beside DESIGN.md 3.17's table: C2 at 512 x 512 and C3 at 1080p, under
           the reference estimator and under cosine bounces with MIS, --frames frames of --spp samples from the seeds frame = 1000 k, under
           JADE_FUSED=0 JADE_TAIL=0 on both sides (the schedule a stratified render runs anyway).  Per estimator and branch sampling:
             variance            the across-frame variance summed over pixels and channels, of the frame
             passes              under the reference estimator (the one the mode keeps passes with): per pass its share of the mean
                                 radiance and its across-frame variance, absolute, so that the two modes' rows can be divided
             outliers            pixel channels of the frame, over all frames, above 8 x (ref + 0.05) - mis_ab.py's rule - with ref one
                                 frame of --ref-spp samples of the RANDOM mode under the same estimator from the seed 900000
             relMSE              at 16, 64 and 256 spp: mean over pixel channels of (x - ref)^2 / (ref^2 + 1e-4), mean over the frames
                                 (4 frames at 256 spp), and `median_rel_sq_err`, the median over pixel channels of the same quantity
             time                ms per sample, --repeats alternating steps of --spp samples plus flush after a warm-up each
           and stratified over random of each.  --bench-parent / --bench-this: files of bench.py result lines (bench.py --gpus 1 --steps 4
           --warmup 1 with JADE_HIP_LIB on the parent's libjade_hip.so, and with this build's, alternating); they go under "bench".
           No threshold: the figures are reported as measured.  A non-parity mode, nobody's default.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# read once, at jade_scene_create: the schedule a stratified render runs, for the random renders too
os.environ["JADE_FUSED"] = "0"
os.environ["JADE_TAIL"] = "0"

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

ESTIMATORS = (("reference", _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS, True), ("cosine+mis", _abi.BOUNCE_COSINE, _abi.DIRECT_MIS, False))
MODES = (("random", _abi.BRANCH_RANDOM), ("stratified", _abi.BRANCH_STRATIFIED))
SIZES = {"C2": (512, 512)}
REL_FLOOR = 1e-4


def scene_of(name):
    hs, cfg = J.build_config(name)

    def make(spp, frame=0):
        p = B.params_from_config(cfg)
        if name in SIZES:
            p.width, p.height = SIZES[name]
        p.spp, p.frame, p.walk = spp, frame, _abi.WALK_EARLY_EXIT
        return p
    return hs, make


def timed(sc, mode, p):
    sc.set_branch_sampling(mode)
    st = _abi.Stats()
    sc.begin(p)
    sc.step(p.spp, st)
    sc.flush(st)
    return dict(kernel_ms=st.kernel_ms, ms_per_sample=st.kernel_ms / p.spp, rays=st.rays, records_per_pixel=sc.query(_abi.Q_RECORDS_PER_PIXEL))


def alternate(sc, p, repeats):
    runs = {name: [] for name, _ in MODES}
    for k in range(repeats + 1):
        for name, mode in MODES:
            r = timed(sc, mode, p)
            if k:
                runs[name].append(r)
    out = {name: dict(runs=rs, ms_per_sample_median=float(np.median([r["ms_per_sample"] for r in rs]))) for name, rs in runs.items()}
    out["stratified_over_random"] = out["stratified"]["ms_per_sample_median"] / out["random"]["ms_per_sample_median"]
    return out


def rel_sq(x, ref):
    return (x - ref) ** 2 / (ref ** 2 + REL_FLOOR)


def figures(sc, make, spp, frames, ref, with_passes):
    """One mode's figures; the handle's branch sampling is set by the caller."""
    bar = 8 * (ref + 0.05)
    f1 = f2 = s1 = s2 = None
    outliers, rel64 = 0, []
    sc.set_passes(with_passes)
    for k in range(1, frames + 1):
        rgb = sc.render(make(spp, frame=1000 * k), want_bgr8=False)[0].astype(np.float64)
        if f1 is None:
            f1, f2 = np.zeros(rgb.shape), np.zeros(rgb.shape)
        f1 += rgb
        f2 += rgb ** 2
        outliers += int((rgb > bar).sum())
        rel64.append(rel_sq(rgb, ref))
        if with_passes:
            ps = np.stack(list(sc.passes().values())).astype(np.float64)
            if s1 is None:
                s1, s2 = np.zeros(ps.shape), np.zeros(ps.shape)
            s1 += ps
            s2 += ps ** 2
    sc.set_passes(False)
    n = float(frames)
    out = dict(variance=float(np.maximum(f2 - f1 ** 2 / n, 0.0).sum() / (n - 1)), outliers=outliers, mean_radiance_per_pixel_channel=float(f1.mean() / n))
    rel = {str(spp): dict(relMSE=float(np.mean([r.mean() for r in rel64])), median_rel_sq_err=float(np.mean([np.median(r) for r in rel64])))}
    for other, count in ((spp // 4, frames), (spp * 4, max(frames // 4, 1))):
        rs = [rel_sq(sc.render(make(other, frame=1000 * k), want_bgr8=False)[0].astype(np.float64), ref) for k in range(1, count + 1)]
        rel[str(other)] = dict(relMSE=float(np.mean([r.mean() for r in rs])), median_rel_sq_err=float(np.mean([np.median(r) for r in rs])), frames=count)
    out["rel"] = rel
    if with_passes:
        var = np.maximum(s2 - s1 ** 2 / n, 0.0).sum(axis=(1, 2, 3)) / (n - 1)
        mean = s1.sum(axis=(1, 2, 3)) / n
        out["passes"] = {name: dict(mean_share=float(mean[i] / mean.sum()), variance=float(var[i]), variance_share=float(var[i] / var.sum()))
                         for i, name in enumerate(_abi.PASS_NAMES)}
    return out


def ratio(a, b):
    return float(a / b) if b else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_ab.json"))
    ap.add_argument("--scenes", default="C2,C3")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "spp": a.spp, "frames": a.frames, "repeats": a.repeats, "ref_spp": a.ref_spp,
           "schedule": {"JADE_FUSED": "0", "JADE_TAIL": "0"}, "scenes": {}}
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
    for name in a.scenes.split(","):
        hs, make = scene_of(name)
        p0 = make(1)
        e = {"width": int(p0.width), "height": int(p0.height), "triangles": int(hs.n_triangles), "emitter_entries": int(len(hs.a["emit"])), "estimators": {}}
        with hip.scene(hs) as sc:
            for est, bounce, direct, with_passes in ESTIMATORS:
                sc.set_bounce_sampling(bounce)
                sc.set_direct_sampling(direct)
                row = dict(time=alternate(sc, make(a.spp), a.repeats))
                sc.set_branch_sampling(_abi.BRANCH_RANDOM)
                ref = sc.render(make(a.ref_spp, frame=900000), want_bgr8=False)[0].astype(np.float64)
                for mode_name, mode in MODES:
                    sc.set_branch_sampling(mode)
                    row[mode_name] = figures(sc, make, a.spp, a.frames, ref, with_passes)
                r, s = row["random"], row["stratified"]
                over = dict(variance=ratio(s["variance"], r["variance"]), outliers=ratio(s["outliers"], r["outliers"]),
                            relMSE={k: ratio(s["rel"][k]["relMSE"], r["rel"][k]["relMSE"]) for k in r["rel"]},
                            median_rel_sq_err={k: ratio(s["rel"][k]["median_rel_sq_err"], r["rel"][k]["median_rel_sq_err"]) for k in r["rel"]})
                if with_passes:
                    over["pass_variance"] = {n: ratio(s["passes"][n]["variance"], r["passes"][n]["variance"]) for n in _abi.PASS_NAMES}
                row["stratified_over_random"] = over
                e["estimators"][est] = row
                print(f"{name} {est}: stratified / random: variance {over['variance']:.3f}, outliers {s['outliers']} / {r['outliers']}, relMSE " +
                      ", ".join(f"{k} spp {v:.3f}" for k, v in sorted(over["relMSE"].items(), key=lambda kv: int(kv[0]))) +
                      f", time x{row['time']['stratified_over_random']:.3f}" +
                      (f"; emission {over['pass_variance']['emission']:.3f}, sss_emitter_first {over['pass_variance']['sss_emitter_first']:.3f}" if with_passes else ""),
                      flush=True)
        res["scenes"][name] = e
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
