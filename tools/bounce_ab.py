"""Cosine-weighted bounce sampling (include/jade_bvh.h: jade_scene_set_bounce_sampling) against the reference's uniform hemisphere: what DESIGN.md 3.12 quotes.

usage: python tools/bounce_ab.py [--out profiles/bounce_ab.json] [--configs C2,C3] [--repeats 3] [--step-spp 8] [--converged-spp 2048] [--frames 2]
           The built-in configurations at their own sizes, the two modes alternating in ONE scene handle, under each environment sampling:
             time     one step of --step-spp samples plus flush, --repeats times per mode after a warm-up each: device time per sample
                      from jade_stats
             noise    relMSE at EQUAL samples per pixel, 16 / 64 / 256, --frames independent frames per mode and count, against the mean
                      of two converged frames, one per mode, of --converged-spp samples each (written down in the result):
                      relMSE = mean over the compared pixels and channels of (x - ref)^2 / (ref^2 + 1e-4).
                      Sky pixels are left out: a pixel whose two converged frames are the same bits reached no sampling vertex in
                      either mode (open sky, an emitter seen directly) and has nothing to compare.
           No threshold: the figures are reported as measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

MODES = (("uniform", _abi.BOUNCE_UNIFORM), ("cosine", _abi.BOUNCE_COSINE))
ENVS = (("reference", _abi.ENV_REFERENCE), ("importance", _abi.ENV_IMPORTANCE))
NOISE_SPP = (16, 64, 256)


def params(cfg, spp, env, frame=0):
    p = B.params_from_config(cfg)
    p.spp, p.frame, p.env_sampling, p.walk = spp, frame, env, _abi.WALK_EARLY_EXIT
    return p


def timed(sc, mode, p):
    sc.set_bounce_sampling(mode)
    st = _abi.Stats()
    sc.begin(p)
    sc.step(p.spp, st)
    sc.flush(st)
    return dict(kernel_ms=st.kernel_ms, ms_per_sample=st.kernel_ms / p.spp, rays=st.rays, rays_env=st.rays_env, rays_indirect=st.rays_indirect,
                nodes_visited=st.nodes_visited, mray_per_s=st.rays / st.kernel_ms / 1e3)


def alternate(sc, p, repeats):
    runs = {name: [] for name, _ in MODES}
    for k in range(repeats + 1):
        for name, mode in MODES:
            r = timed(sc, mode, p)
            if k:
                runs[name].append(r)
    return {name: dict(runs=rs, ms_per_sample_median=float(np.median([r["ms_per_sample"] for r in rs]))) for name, rs in runs.items()}


def rel_mse(x, ref, keep):
    x, ref = x.astype(np.float64)[keep], ref.astype(np.float64)[keep]
    return float(((x - ref) ** 2 / (ref ** 2 + 1e-4)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounce_ab.json"))
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-spp", type=int, default=8)
    ap.add_argument("--converged-spp", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=2)
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "repeats": a.repeats, "converged_spp_per_mode": a.converged_spp, "frames": a.frames, "configs": {}}
    for name in a.configs.split(","):
        hs, cfg = J.build_config(name)
        out = {"width": int(cfg.width), "height": int(cfg.height), "triangles": int(hs.n_triangles), "emitter_entries": int(len(hs.a["emit"]))}
        with hip.scene(hs) as sc:
            for env_name, env in ENVS:
                e = {}
                try:
                    e["time"] = dict(spp=a.step_spp, **alternate(sc, params(cfg, a.step_spp, env), a.repeats))
                except B.JadeError as err:
                    out[env_name] = {"refused": str(err)}
                    continue
                conv = {}
                for mode_name, mode in MODES:
                    sc.set_bounce_sampling(mode)
                    conv[mode_name] = sc.render(params(cfg, a.converged_spp, env, frame=900000), want_bgr8=False)[0]
                ref = 0.5 * (conv["uniform"].astype(np.float64) + conv["cosine"].astype(np.float64))
                keep = ~(conv["uniform"].view(np.uint32) == conv["cosine"].view(np.uint32)).all(-1)
                e["compared_pixels"] = int(keep.sum())
                e["converged_frames_rel_difference"] = rel_mse(conv["cosine"], conv["uniform"], keep)
                e["converged_total_cosine_over_uniform"] = float(conv["cosine"].astype(np.float64)[keep].sum() / conv["uniform"].astype(np.float64)[keep].sum())
                e["noise"] = {}
                for spp in NOISE_SPP:
                    row = {}
                    for mode_name, mode in MODES:
                        sc.set_bounce_sampling(mode)
                        v = [rel_mse(sc.render(params(cfg, spp, env, frame=1000 * k), want_bgr8=False)[0], ref, keep) for k in range(1, a.frames + 1)]
                        row[mode_name] = dict(rel_mse=v, rel_mse_mean=float(np.mean(v)))
                    row["rel_mse_cosine_over_uniform"] = row["cosine"]["rel_mse_mean"] / row["uniform"]["rel_mse_mean"]
                    e["noise"][str(spp)] = row
                out[env_name] = e
                t = e["time"]
                print(f"{name} env {env_name}: ms per sample uniform {t['uniform']['ms_per_sample_median']:.3f} cosine {t['cosine']['ms_per_sample_median']:.3f}; "
                      "relMSE cosine / uniform at " + ", ".join(f"{s} spp {e['noise'][str(s)]['rel_mse_cosine_over_uniform']:.3f}" for s in NOISE_SPP) +
                      f"; converged totals cosine / uniform {e['converged_total_cosine_over_uniform']:.5f} over {e['compared_pixels']} pixels", flush=True)
        res["configs"][name] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
