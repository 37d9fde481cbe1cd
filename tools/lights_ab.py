"""One-light sampling (include/jade_bvh.h: jade_scene_set_light_sampling) against the all-lights loop: what DESIGN.md 3.11 quotes.

usage: python tools/lights_ab.py [--out profiles/lights_ab.json] [--repeats 3] [--noise-spp 16] [--frames 4]
           Two scenes - a slab, a ball and a jade box under a geodesic lamp of 80 / 1280 triangles and two quad lights (84 / 1284 emitter
           entries) - in both modes:
             time     1920 x 1080 (C3's frame), one step of a few samples plus flush, the modes alternating, --repeats times each after a
                      warm-up: device time per sample from jade_stats, and the records per pixel the render got
             noise    256 x 256 (C1's frame): --frames independent frames per mode, all lights at --noise-spp samples and one light at as
                      many samples as take the same device time (from times measured at this size), against the mean of two converged
                      frames, one per mode: relMSE = mean over the lit pixels and channels of (x - ref)^2 / (ref^2 + 1e-4)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B, host as H  # noqa: E402

MODES = (("all", _abi.LIGHTS_ALL), ("one", _abi.LIGHTS_ONE))
QUAD_I = np.int32([[0, 1, 2], [0, 2, 3]])
# (lamp frequency: 20 f^2 triangles, samples of the timed step at 1080p, samples of the converged frames: all lights, one light)
SCENES = {"84 entries": (2, 16, 2048, 16384), "1284 entries": (8, 4, 1024, 32768)}


def build(freq):
    """tests/test_gpu_lights.py's scene."""
    b = H.SceneBuilder()
    try:
        T = H.transform_matrix
        jade = H.material(brdf=(0.3, 0.4, 0.5), reflex_mode=_abi.MIRROR, refract_mode=_abi.SUB_SURFACE, refract_rate=(0.3, 0.4, 0.5),
                          refract_albedo=(0.3, 0.5, 0.7), refract_index=2.66)
        b.add_proc("box", 0, H.material(brdf=(0.6, 0.5, 0.4)), T(trans=(0, -1.1, 0), scale=(7, 0.2, 7)))
        b.add_proc("geodesic", 2, H.material(brdf=(0.5, 0.6, 0.5)), T(trans=(-1.1, -0.45, 0.2), scale=(0.5,) * 3))
        b.add_proc("box", 0, jade, T(rot_deg=(0, 35, 0), trans=(0.55, -0.7, 0.9), scale=(0.6,) * 3))
        b.add_proc("geodesic", freq, H.material(emissive=(30, 27, 22), brdf=(0.3,) * 3), T(trans=(0.3, 1.3, 0.4), scale=(0.25,) * 3))
        big = np.float32([[-2.6, 0.2, -1.8], [-1.4, 0.2, -1.8], [-1.4, 1.4, -1.8], [-2.6, 1.4, -1.8]])
        b.add_mesh(big, QUAD_I, H.material(emissive=(9, 12, 15), brdf=(0.3,) * 3))
        small = np.float32([[1.8, -0.6, 1.6], [2.1, -0.6, 1.3], [2.1, -0.3, 1.3], [1.8, -0.3, 1.6]])
        b.add_mesh(small, QUAD_I, H.material(emissive=(40, 10, 4), brdf=(0.3,) * 3))
        b.set_env_sky(16, 8)
        return b.build()
    finally:
        b.close()


def params(w, h, spp, frame=0):
    eye, cam = H.camera_orbit(5.0, 20.0, 30.0)
    return B.make_params(w, h, spp, eye, cam, frame=frame, walk=_abi.WALK_EARLY_EXIT)


def timed(sc, mode, p):
    sc.set_light_sampling(mode)
    st = _abi.Stats()
    sc.begin(p)
    rpp = sc.query(_abi.Q_RECORDS_PER_PIXEL)
    sc.step(p.spp, st)
    sc.flush(st)
    return dict(kernel_ms=st.kernel_ms, ms_per_sample=st.kernel_ms / p.spp, records_per_pixel=rpp, rays=st.rays, rays_shadow=st.rays_shadow,
                rays_env=st.rays_env, mray_per_s=st.rays / st.kernel_ms / 1e3)


def alternate(sc, p, repeats):
    """Both modes `repeats` times, alternating, after one warm-up each: {mode: {runs, median ms per sample, records per pixel}}."""
    runs = {name: [] for name, _ in MODES}
    for k in range(repeats + 1):
        for name, mode in MODES:
            r = timed(sc, mode, p)
            if k:
                runs[name].append(r)
    return {name: dict(runs=rs, ms_per_sample_median=float(np.median([r["ms_per_sample"] for r in rs])),
                       records_per_pixel=rs[0]["records_per_pixel"]) for name, rs in runs.items()}


def rel_mse(x, ref, lit):
    x, ref = x.astype(np.float64)[lit], ref.astype(np.float64)[lit]
    return float(((x - ref) ** 2 / (ref ** 2 + 1e-4)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lights_ab.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--noise-spp", type=int, default=16)
    ap.add_argument("--frames", type=int, default=4)
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "repeats": a.repeats, "scenes": {}}
    for label, (freq, step_spp, conv_all, conv_one) in SCENES.items():
        hs = build(freq)
        out = {"triangles": int(hs.n_triangles), "emitter_entries": int(len(hs.a["emit"]))}
        with hip.scene(hs) as sc:
            out["time_1920x1080"] = dict(spp=step_spp, **alternate(sc, params(1920, 1080, step_spp), a.repeats))
            # (a render never gets more records per pixel than samples it announces: asked again for a 4096-sample render, begin only)
            out["records_per_pixel_1920x1080_4096spp"] = {}
            for name, mode in MODES:
                sc.set_light_sampling(mode)
                sc.begin(params(1920, 1080, 4096))
                out["records_per_pixel_1920x1080_4096spp"][name] = sc.query(_abi.Q_RECORDS_PER_PIXEL)
            small = alternate(sc, params(256, 256, a.noise_spp), a.repeats)
            ratio = small["all"]["ms_per_sample_median"] / small["one"]["ms_per_sample_median"]
            spp_one = max(1, int(round(a.noise_spp * ratio)))
            conv = {}
            for (name, mode), spp in zip(MODES, (conv_all, conv_one)):
                sc.set_light_sampling(mode)
                conv[name] = sc.render(params(256, 256, spp, frame=900000))[0]
            ref = 0.5 * (conv["all"].astype(np.float64) + conv["one"].astype(np.float64))
            lit = (conv["all"] < 4).all(-1)  # not straight into a lamp (tests/test_gpu_lights.py)
            noise = {}
            for (name, mode), spp in zip(MODES, (a.noise_spp, spp_one)):
                sc.set_light_sampling(mode)
                if name == "one":
                    # a step's fixed cost weighs on the short timed steps above: one trial frame, then the samples scaled to the time the
                    # all-lights frames really took
                    trial = sc.render(params(256, 256, spp, frame=800000))[2].kernel_ms
                    spp = max(1, int(round(spp * float(np.mean(noise["all"]["kernel_ms"])) / trial)))
                frames, ms = [], []
                for k in range(1, a.frames + 1):
                    rgb, _, st = sc.render(params(256, 256, spp, frame=1000 * k))
                    frames.append(rel_mse(rgb, ref, lit))
                    ms.append(st.kernel_ms)
                noise[name] = dict(spp=spp, rel_mse=frames, rel_mse_mean=float(np.mean(frames)), kernel_ms=ms)
            out["noise_256x256"] = dict(time=small, converged_spp=dict(all=conv_all, one=conv_one), lit_pixels=int(lit.sum()),
                                        converged_frames_rel_difference=rel_mse(conv["one"], conv["all"], lit),
                                        total_one_over_all=float(conv["one"].astype(np.float64)[lit].sum() / conv["all"].astype(np.float64)[lit].sum()),
                                        equal_time=noise, rel_mse_one_over_all=noise["one"]["rel_mse_mean"] / noise["all"]["rel_mse_mean"])
        res["scenes"][label] = out
        t = out["time_1920x1080"]
        n = out["noise_256x256"]
        print(f"{label}: 1080p ms per sample all {t['all']['ms_per_sample_median']:.2f} one {t['one']['ms_per_sample_median']:.2f} "
              f"({t['all']['ms_per_sample_median'] / t['one']['ms_per_sample_median']:.1f}x); records per pixel of a 4096-spp render all {out['records_per_pixel_1920x1080_4096spp']['all']} "
              f"one {out['records_per_pixel_1920x1080_4096spp']['one']}; equal time at 256x256: all {n['equal_time']['all']['spp']} spp relMSE "
              f"{n['equal_time']['all']['rel_mse_mean']:.4g}, one {n['equal_time']['one']['spp']} spp relMSE {n['equal_time']['one']['rel_mse_mean']:.4g} "
              f"(one / all {n['rel_mse_one_over_all']:.2f}); converged totals one / all {n['total_one_over_all']:.4f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
