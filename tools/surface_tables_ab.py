"""The surface-table refactor against its parent commit's build of the HIP library, on one machine in one session, the
two builds alternating: what profiles/surface_tables_ab.json holds.

usage: python tools/surface_tables_ab.py --parent-lib PATH/libjade_hip.so [--repeats 5] [--commit ID --parent-commit ID] [--out FILE]
  bench    `python bench.py` with its defaults, a process per run, the parent's library through JADE_HIP_LIB: Mray/s and frame_sha256.
           Nothing on that path changed, so the frame hash must be one and this build's median must lie inside the parent's min .. max.
  guides   the wall time of Scene.guides(4) at 512 x 512 after a 1-spp render of tests/test_gpu_guide_tables_exact.py's scene, in each of
           its six handle states, both libraries loaded in this process; the call ends in copies to the host, so the clock stops after the
           device has.  One untimed call per state and build first; which build goes first alternates from repeat to repeat.  This
           build's median is accepted within the parent's own spread (max - min) of the parent's median.  The guides of the two builds
           are compared bit for bit as well.
No threshold is enforced here: the figures are written down as measured, with "within" per line.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from jaderaytracerendering_amd import backend as B, host as H  # noqa: E402


def bench_once(lib):
    env = dict(os.environ)
    if lib:
        env["JADE_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if out.returncode:
        raise SystemExit(f"bench.py failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    r = json.loads(line)
    return {"value": r["value"], "frame_sha256": r["frame_sha256"]}


def spread(xs):
    return {"runs": xs, "median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def bench_ab(parent_lib, repeats):
    runs = {"parent": [], "this": []}
    for k in range(repeats):
        for who, lib in (("parent", parent_lib), ("this", None)):
            runs[who].append(bench_once(lib))
            print(f"bench {k} {who}: {runs[who][-1]['value']:.1f} Mray/s", flush=True)
    out = {who: spread([r["value"] for r in rs]) for who, rs in runs.items()}
    hashes = {r["frame_sha256"] for rs in runs.values() for r in rs}
    out["frame_sha256"] = sorted(hashes)
    out["one_frame_hash"] = len(hashes) == 1
    out["within"] = out["parent"]["min"] <= out["this"]["median"] <= out["parent"]["max"]
    return out


def guides_ab(parent_lib, repeats, size=512, guide_spp=4):
    import test_gpu_guide_tables_exact as T
    builds = {"parent": B.Backend(parent_lib), "this": B.hip()}
    eye, cam = H.camera_orbit(2.0, T.UP_DEG, T.ROT_DEG)
    p = B.make_params(size, size, 1, eye, cam, frame=T.FRAME)
    out = {}
    for state in T.STATES:
        hs, _ = T.scene(state)
        ms = {"parent": [], "this": []}
        sha = {}
        scenes = {who: be.scene(hs) for who, be in builds.items()}
        try:
            for who, sc in scenes.items():
                sc.render(p)
                g = sc.guides(guide_spp)  # untimed: allocations, code objects
                sha[who] = hashlib.sha256(b"".join(np.ascontiguousarray(g[k]).tobytes() for k in ("albedo", "normal", "depth"))).hexdigest()
            for k in range(repeats):
                for who, sc in (list(scenes.items())[::-1] if k % 2 else scenes.items()):  # (who goes first alternates as well)
                    t0 = time.perf_counter()
                    sc.guides(guide_spp)
                    ms[who].append((time.perf_counter() - t0) * 1e3)
        finally:
            for sc in scenes.values():
                sc.close()
        e = {who: spread(v) for who, v in ms.items()}
        e["same_bits"] = sha["parent"] == sha["this"]
        e["within"] = abs(e["this"]["median"] - e["parent"]["median"]) <= e["parent"]["max"] - e["parent"]["min"]
        out[state] = e
        print(f"guides, {state}: parent {e['parent']['median']:.3f} ms ({e['parent']['min']:.3f} .. {e['parent']['max']:.3f}), this {e['this']['median']:.3f} ms "
              f"({e['this']['min']:.3f} .. {e['this']['max']:.3f}), same bits {e['same_bits']}, within {e['within']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--guide-repeats", type=int, default=15)
    ap.add_argument("--commit", default="")
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_tables_ab.json"))
    args = ap.parse_args()
    parent_lib = os.path.abspath(args.parent_lib)
    rec = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "commit": args.commit, "parent_commit": args.parent_commit,
           "repeats": args.repeats, "guide_repeats": args.guide_repeats,
           "guides_ms": guides_ab(parent_lib, args.guide_repeats), "bench_mray_s": bench_ab(parent_lib, args.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
