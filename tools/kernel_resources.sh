#!/bin/bash
# Per-kernel register / LDS / scratch / occupancy of the HIP module as hipcc reports them (-Rpass-analysis=kernel-resource-usage).
# usage: tools/kernel_resources.sh [extra -D flags...]      (JADE_RESOURCE_FILES="jade_despeckle ..." lists those files only)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
for f in ${JADE_RESOURCE_FILES:-jade_hip jade_bvh jade_adaptive jade_denoise jade_expose jade_glare jade_passes jade_despeckle}; do
/opt/rocm/bin/hipcc "$@" -O3 -fno-slp-vectorize -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math \
  -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -mfma -I"$R/include" -I"$R/jaderaytracerendering_amd/csrc" \
  -c "$R/jaderaytracerendering_amd/csrc/$f.hip" -o "$T/x.o" -Rpass-analysis=kernel-resource-usage 2>&1 |
  python3 -c '
import re, sys
cur = None
rows = {}
for line in sys.stdin:
    m = re.search(r"remark:\s+Function Name: (\S+)", line)
    if m:
        cur = m.group(1); rows[cur] = {}; continue
    m = re.search(r"remark:\s+([A-Za-z /\[\]]+): ([0-9]+)", line)
    if m and cur:
        rows[cur][m.group(1).strip()] = int(m.group(2))
for k, v in rows.items():
    m = re.match(r"^_Z\d+(k_[a-z_0-9]+?)(?=\d|P|$)", k)
    t = re.match(r"^_Z\d+(k_[a-z_0-9]+)ILb([01])EE", k)  # a kernel template over one bool: k_name<0> / k_name<1>
    s = re.match(r"^_Z\d+(k_[a-z_0-9]+)ILj(\d+)E", k)  # a kernel template over the ShadeMode mask (jade_runtime.h): k_shade_mode<COSINE|MIS>
    n = re.match(r"^_Z\d+(k_[a-z_0-9]+)ILi(\d+)E", k)  # a kernel template over one int: k_despeckle<2>
    if not m and not t and not s and not n:
        continue
    bits = ("ENVIS", "LENS", "SHUTTER", "LIGHTS", "COSINE", "MIS", "ENVMIX", "PASSES", "BRANCH", "SMOOTH", "TEX", "NMAP")
    if n:
        name = "%s<%s>" % (n.group(1), n.group(2))
    elif s:
        name = "%s<%s>" % (s.group(1), "|".join(b for i, b in enumerate(bits) if int(s.group(2)) >> i & 1) or "0")
    else:
        name = "%s<%s>" % (t.group(1), t.group(2)) if t else m.group(1)
    print("%-16s VGPR %3d AGPR %3d SGPR %3d scratch %4d B  LDS %6d B  occupancy %d" % (name, v.get("VGPRs", -1), v.get("AGPRs", 0), v.get("TotalSGPRs", v.get("SGPRs", -1)), v.get("ScratchSize [bytes/lane]", v.get("ScratchSize", 0)), v.get("LDS Size [bytes/block]", v.get("LDS Size", 0)), v.get("Occupancy [waves/SIMD]", v.get("Occupancy", -1))))
'
done
