"""Where a frame's radiance, variance and rare bright samples come from, pass by pass (include/jade_bvh.h: jade_scene_set_passes, jade_render_passes): what DESIGN.md 3.17 and 7 quote.

usage: python tools/passes_ab.py [--out profiles/passes_ab.json] [--scenes C2,C3] [--spp 64] [--frames 16] [--repeats 3]
                                 [--bench-parent FILE --bench-this FILE]
           C2 at 512 x 512 and C3 at 1080p, under the reference estimator and under cosine bounces with MIS, --frames frames of --spp samples
           from the seeds frame = 1000 k, passes kept.  Per estimator and pass:
             mean_share      the pass's share of the mean radiance (summed over pixels and channels, mean over the frames)
             variance_share  its share of the across-frame variance summed over pixels and channels (the passes' variances; their
                             covariances are what `variance_of_frame_over_sum_of_passes` differs from 1 by)
             outliers        pixel channels of the pass, over all frames, above 8 x (ref + 0.05) - mis_ab.py's definition - with ref one
                             frame of frames x spp samples under the same estimator from the seed 900000; `frame_outliers` is the
                             same count on the frame itself.  Where ref is below -0.05 (negative radiance: the reference's
                             schlick_out) the bar is negative and every pass, a pass of 0 included, is above it in every frame:
                             `negative_bar_channel_frames` is that floor, to be subtracted from every count
           and the cost of a sample with passes against without under the same schedule (the tool runs under JADE_FUSED=0 JADE_TAIL=0, the
           schedule a passes render runs anyway): --repeats alternating steps of --spp samples plus flush after a warm-up each.
           --bench-parent / --bench-this: files of bench.py result lines (one JSON object per run: bench.py --gpus 1 --steps 4 --warmup 1 with
           JADE_HIP_LIB on the parent's libjade_hip.so, and with this build's, alternating); their headline, step time, frame hash and ray
           count go under "bench".  Without them a "bench" entry the output file already has is kept.
           No threshold: the figures are reported as measured.  A diagnosis mode, nobody's default.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# read once, at jade_scene_create: the schedule a passes render runs, for the renders without passes too
os.environ["JADE_FUSED"] = "0"
os.environ["JADE_TAIL"] = "0"

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

ESTIMATORS = (("reference", _abi.BOUNCE_UNIFORM, _abi.DIRECT_RAYS), ("cosine+mis", _abi.BOUNCE_COSINE, _abi.DIRECT_MIS))
SIZES = {"C2": (512, 512)}


def scene_of(name):
    hs, cfg = J.build_config(name)

    def make(spp, frame=0):
        p = B.params_from_config(cfg)
        if name in SIZES:
            p.width, p.height = SIZES[name]
        p.spp, p.frame, p.walk = spp, frame, _abi.WALK_EARLY_EXIT
        return p
    return hs, make


def timed(sc, on, p):
    sc.set_passes(on)
    st = _abi.Stats()
    sc.begin(p)
    sc.step(p.spp, st)
    sc.flush(st)
    return dict(kernel_ms=st.kernel_ms, ms_per_sample=st.kernel_ms / p.spp, rays=st.rays, records_per_pixel=sc.query(_abi.Q_RECORDS_PER_PIXEL))


def alternate(sc, p, repeats):
    runs = {"without": [], "with": []}
    for k in range(repeats + 1):
        for name, on in (("without", False), ("with", True)):
            r = timed(sc, on, p)
            if k:
                runs[name].append(r)
    out = {name: dict(runs=rs, ms_per_sample_median=float(np.median([r["ms_per_sample"] for r in rs]))) for name, rs in runs.items()}
    out["with_over_without"] = out["with"]["ms_per_sample_median"] / out["without"]["ms_per_sample_median"]
    return out


def split_of(sc, make, spp, frames):
    """Running sums over the frames: of the frame, of every pass and of their squares."""
    s1 = s2 = f1 = f2 = None
    sc.set_passes(False)
    ref = sc.render(make(spp * frames, frame=900000), want_bgr8=False)[0].astype(np.float64)
    sc.set_passes(True)
    bar = (8 * (ref + 0.05)).astype(np.float32)
    outliers = np.zeros(len(_abi.PASS_NAMES), np.int64)
    frame_outliers = 0
    for k in range(1, frames + 1):
        rgb = sc.render(make(spp, frame=1000 * k), want_bgr8=False)[0].astype(np.float64)
        ps = np.stack(list(sc.passes().values())).astype(np.float32)
        if s1 is None:
            s1, s2, f1, f2 = np.zeros(ps.shape), np.zeros(ps.shape), np.zeros(rgb.shape), np.zeros(rgb.shape)
        s1 += ps
        s2 += ps.astype(np.float64) ** 2
        f1 += rgb
        f2 += rgb ** 2
        outliers += (ps > bar[None]).sum(axis=(1, 2, 3))
        frame_outliers += int((rgb > bar).sum())
    n = float(frames)
    var = np.maximum(s2 - s1 ** 2 / n, 0.0).sum(axis=(1, 2, 3)) / (n - 1)
    var_frame = float(np.maximum(f2 - f1 ** 2 / n, 0.0).sum() / (n - 1))
    mean = s1.sum(axis=(1, 2, 3)) / n
    rows = {name: dict(mean_share=float(mean[i] / mean.sum()), variance_share=float(var[i] / var.sum()), outliers=int(outliers[i]))
            for i, name in enumerate(_abi.PASS_NAMES)}
    return dict(passes=rows, frame_outliers=frame_outliers, negative_bar_channel_frames=int((bar <= 0).sum()) * frames, mean_radiance_per_pixel_channel=float(f1.mean() / n),
                sum_of_passes_over_frame=float(mean.sum() / (f1.sum() / n)), variance_of_frame_over_sum_of_passes=var_frame / float(var.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "passes_ab.json"))
    ap.add_argument("--scenes", default="C2,C3")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "spp": a.spp, "frames": a.frames, "repeats": a.repeats,
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
            for est, bounce, direct in ESTIMATORS:
                sc.set_bounce_sampling(bounce)
                sc.set_direct_sampling(direct)
                row = dict(time=alternate(sc, make(a.spp), a.repeats))
                sc.set_passes(True)
                row.update(split_of(sc, make, a.spp, a.frames))
                e["estimators"][est] = row
                top = sorted(row["passes"].items(), key=lambda kv: -kv[1]["variance_share"])[:4]
                print(f"{name} {est}: a sample costs x{row['time']['with_over_without']:.2f} with passes; variance by pass: " +
                      ", ".join(f"{n} {v['variance_share']:.3f} (mean {v['mean_share']:.3f}, {v['outliers']} outliers)" for n, v in top) +
                      f"; frame outliers {row['frame_outliers']}", flush=True)
        res["scenes"][name] = e
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
