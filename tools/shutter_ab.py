"""Camera shutter (include/jade_bvh.h: jade_scene_set_shutter): what DESIGN.md 3.10 quotes.

usage: python tools/shutter_ab.py [--out profiles/shutter_ab.json] [--spp 1024] [--repeats 3]
           C3 at 1080p, one step of --spp samples plus flush, three ways: under a shutter - a turntable step of 2 degrees about the
           statue; the pinhole under JADE_FUSED=0 JADE_TAIL=0 - the shutter's own schedule, with the parent's kernels; the pinhole
           under the default schedule.  Each way in a scene handle of its own (the switches are read at jade_scene_create), --repeats
           times, device times from jade_stats.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B, host as H  # noqa: E402

WIDTH, HEIGHT = 1920, 1080
ORBIT_DEG = 2.0
PIVOT = (0.26, -1.28, 0.0)  # the centre C3's camera orbits (host/scene_io.cpp)
SWITCHES = ("JADE_FUSED", "JADE_TAIL")


def built(config):
    b = J.SceneBuilder()
    try:
        cfg = b.config(config)
        hs = b.build()
    finally:
        b.close()
    return hs, cfg


def one_way(hip, hs, p, shutter, env, spp, repeats):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    runs = []
    with hip.scene(hs) as sc:
        if shutter:
            sc.set_shutter(*shutter)
        for _ in range(repeats + 1):  # the first allocates: left out
            st = _abi.Stats()
            t0 = time.perf_counter()
            sc.begin(p)
            sc.step(spp, st)
            sc.flush(st)
            wall = (time.perf_counter() - t0) * 1e3
            shade = st.kernel_ms - st.trace_ms - st.light_ms - st.tail_ms
            runs.append(dict(wall_ms=wall, kernel_ms=st.kernel_ms, k_trace_ms=st.trace_ms, first_pass_ms=st.light_ms, k_tail_ms=st.tail_ms,
                             shading_and_rest_ms=shade, rays=st.rays, rays_primary=st.rays_primary, rays_inline=st.rays_inline,
                             nodes_visited=st.nodes_visited, trace_launches=st.trace_launches, mray_per_s=st.rays / st.kernel_ms / 1e3))
    for k in SWITCHES:
        os.environ.pop(k, None)
    runs = runs[1:]
    best = min(runs, key=lambda r: r["kernel_ms"])
    return dict(env=env, shutter=bool(shutter), runs=runs, kernel_ms_median=float(np.median([r["kernel_ms"] for r in runs])), fastest=best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter_ab.json"))
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    hip = J.hip()
    hs, cfg = built("C3")
    p = B.params_from_config(cfg, spp=a.spp, walk=_abi.WALK_EARLY_EXIT)
    p.width, p.height = WIDTH, HEIGHT
    eye, cam = np.array(p.eye[:], np.float32), np.array(p.camera[:], np.float32)
    close = H.camera_move(eye, cam, orbit_deg=ORBIT_DEG, pivot=PIVOT)
    res = {"what": __doc__.strip().splitlines()[0], "config": "C3", "width": WIDTH, "height": HEIGHT, "spp": a.spp, "repeats": a.repeats,
           "shutter": dict(orbit_deg=ORBIT_DEG, pivot=PIVOT, t_open=0.0, t_close=1.0), "ways": {}}
    res["ways"]["shutter"] = one_way(hip, hs, p, close, {}, a.spp, a.repeats)
    res["ways"]["pinhole, the shutter's schedule (JADE_FUSED=0 JADE_TAIL=0)"] = one_way(hip, hs, p, None, {"JADE_FUSED": "0", "JADE_TAIL": "0"}, a.spp, a.repeats)
    res["ways"]["pinhole, default schedule"] = one_way(hip, hs, p, None, {}, a.spp, a.repeats)
    for k, v in res["ways"].items():
        b = v["fastest"]
        print(f"{k}: kernel {v['kernel_ms_median']:.1f} ms median ({', '.join('%.1f' % r['kernel_ms'] for r in v['runs'])}); fastest: k_trace "
              f"{b['k_trace_ms']:.1f}, first pass {b['first_pass_ms']:.1f}, k_tail {b['k_tail_ms']:.1f}, shading and rest {b['shading_and_rest_ms']:.1f} ms; "
              f"{b['rays'] / 1e9:.3f} Grays, {b['mray_per_s']:.0f} Mray/s, {b['nodes_visited'] / b['rays']:.1f} nodes per ray", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
