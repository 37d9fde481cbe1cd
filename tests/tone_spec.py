"""The tone curve, stated independently in float64 numpy, and the inputs its tests share.

Written from the reference's text, not from the oracle or the HIP module:
  * ACESToneMapping, PathTrace.cu:674-682:  a = x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14)   per channel
  * toneMapping(c, limit), PathTrace.cu:669-672 == pass3.fsh:8-18:  a = x / (1 + (0.3 r + 0.6 g + 0.1 b) / limit)
  * the pack, PathTrace.cu:1461-1473:  byte = float -> uchar of min(255 a^(1/2.2), 255), written B G R; DESIGN.md section 2 defines
    the conversion of a NaN or a negative value as 0.
The ACES denominator is positive for every finite x (its discriminant 0.59^2 - 4 * 2.43 * 0.14 is negative), so nothing is excluded.
"""
import numpy as np

ACES, REINHARD = 0, 1  # include/jade_rt.h, JADE_TONEMAP_*


def curve(rgb, tonemap, limit):
    """The unclamped value 255 a^(1/2.2) of every channel of float32 rgb [n, 3], float64 [n, 3]; NaN where a is non-positive or a NaN."""
    x = np.asarray(rgb, np.float64)
    with np.errstate(all="ignore"):
        if tonemap == REINHARD:
            lum = 0.3 * x[:, 0] + 0.6 * x[:, 1] + 0.1 * x[:, 2]
            a = x * (1.0 / (1.0 + lum / np.float64(np.float32(limit))))[:, None]
        else:
            a = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)
        return 255.0 * np.power(np.where(a > 0, a, np.nan), 1.0 / 2.2)  # (IEEE pow(-inf, 1 / 2.2) would be +inf)


def expected_bytes(rgb, tonemap, limit):
    """(bgr uint8 [n, 3], near bool [n, 3] in B G R order): floor(min(v, 255)) of the curve, 0 for a non-positive or NaN value;
    near marks the values strictly between 0 and 255 that lie within 1e-3 of an integer k = 1 .. 255 - the points where the byte
    changes (at k = 255 from below only: from 255 on the statement is clamped and the byte must be 255; 0 is no such point, the
    byte is 0 on both sides of it) - where an fp32 evaluation may land on the other side (jade_powf is tested to 6 ulp: about 2e-4 at 255; 1e-3 is five times that)."""
    v = curve(rgb, tonemap, limit)
    ok = v > 0  # False for NaN
    byte = np.where(ok, np.floor(np.minimum(np.where(ok, v, 0.0), 255.0)), 0.0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        near = ok & (v < 255.0) & (np.rint(v) >= 1) & (np.abs(v - np.rint(v)) <= 1e-3)
    return byte[:, ::-1].copy(), near[:, ::-1].copy()


def _aces_inverse(a):
    """x >= 0 with ACES(x) = a: the positive root of (2.51 - 2.43 a) x^2 + (0.03 - 0.59 a) x - 0.14 a = 0."""
    qa, qb, qc = 2.51 - 2.43 * a, 0.03 - 0.59 * a, -0.14 * a
    return (-qb + np.sqrt(qb * qb - 4 * qa * qc)) / (2 * qa)


def _code_probes(tonemap, limit):
    """For every code c = 0 .. 255 the inputs whose curve value is c - 1e-4, c and c + 1e-4 (one per channel of a row for ACES,
    three grey rows for Reinhard), computed in float64."""
    c = np.arange(0, 256, dtype=np.float64)
    v = np.stack([c - 1e-4, c, c + 1e-4], -1)  # [256, 3]
    a = np.maximum(v, 0.0) / 255.0
    a = a ** 2.2
    if tonemap == ACES:
        return _aces_inverse(a)
    x = a / (1.0 - a / limit)  # grey: lum = x (0.3 + 0.6 + 0.1)
    return np.repeat(x.reshape(-1, 1), 3, 1)


def inputs(tonemap, limit=1.5):
    """About 300 k float32 rgb rows, the finite ones first: (rgb [n, 3], n_generated) - rows [:n_generated] are the generated inputs
    (greys, random triples, negatives), the rest the per-code probes and the special values."""
    rng = np.random.default_rng(21 + tonemap)
    grey = np.repeat(np.linspace(0.0, 16.0, 120001).reshape(-1, 1), 3, 1)
    rnd = rng.random((150000, 3)) * 10.0 ** rng.uniform(-6, 2, (150000, 1))
    neg = rng.normal(size=(30000, 3)) * 10.0 ** rng.uniform(-4, 1, (30000, 1))
    generated = np.concatenate([grey, rnd, neg])
    nan, inf = np.nan, np.inf
    special = [(s if k == ch else 0.5) for s in (nan, inf, -inf, 1e30, -1e30, 3.4e38, -0.0, 1e-45) for ch in range(3) for k in range(3)]
    special = np.array(special).reshape(-1, 3)
    both = np.array([(nan, nan, nan), (inf, inf, inf), (-inf, -inf, -inf), (inf, -inf, nan), (1e30, 1e30, 1e30), (0, 0, 0)])
    rows = [generated, special, both]
    if tonemap == ACES or limit > 1.0:  # (the grey inverse image of a code needs a < limit)
        rows.append(_code_probes(tonemap, limit))
    if tonemap == REINHARD:
        # 1 + lum / limit exactly zero (limit 1.5: 0.6 * -2.5 = -1.5 exactly; the tiny red does not move the sum) and negative
        rows.append(np.array([(0, -2.5, 0), (1e-30, -2.5, 0), (0, -2.5, 1e-30), (0, -5.0, 0), (1.0, -5.0, 0.25), (-1.0, -5.0, 1.0)]))
    return np.concatenate(rows).astype(np.float32), len(generated)


CASES = ((ACES, 0.0), (REINHARD, 1.5), (REINHARD, 1e-30), (REINHARD, 0.0))  # (operator, limit): the default, tiny and zero limits


def check_bytes(got, rgb, tonemap, limit, n_generated):
    """The assertions of tests/test_tone_spec.py (oracle) and tests/test_gpu_tone.py (device) against the float64 statement.
    Returns (share of the generated values inside the allowance, number of bytes that used it)."""
    want, near = expected_bytes(rgb, tonemap, limit)
    finite = np.isfinite(rgb).all(1)[:, None]  # the statement is asserted for finite inputs; the others are compared between the backends
    diff = np.where(finite, got.astype(np.int32) - want.astype(np.int32), 0)
    bad = (diff != 0) & ~(near & (np.abs(diff) == 1))
    if bad.any():
        i = np.argwhere(bad)[:5]
        v = curve(rgb, tonemap, limit)[:, ::-1]
        raise AssertionError(f"tonemap {tonemap}, limit {limit}: {int(bad.sum())} bytes differ from the float64 statement; (row, rgb, "
                             f"channel, got, want, value): {[(int(r), rgb[r].tolist(), int(c), int(got[r, c]), int(want[r, c]), float(v[r, c])) for r, c in i]}")
    share = float(near[:n_generated].mean())
    used = int((diff != 0).sum())
    print(f"tonemap {tonemap} limit {limit}: {used} of {diff.size} bytes off by one (all within 1e-3 of an integer); "
          f"{share:.4%} of the generated values lie inside that allowance")
    assert near.mean() <= 0.02 and share <= 0.02
    return share, used


SPECIAL_ROWS = np.float32([(np.nan, 0.5, 0.5), (0.5, np.nan, -1.0), (np.inf, 1e30, 3.4e38), (-np.inf, -1e30, -0.0), (0, 0, 0), (16, 16, 16)])


def special_bytes():
    """float -> uchar of a NaN or a negative value is 0 (ACES(-1) = 1.25 is not negative); huge and infinite
    values of either sign saturate at 255 (ACES tends to 2.51 / 2.43 on both sides)."""
    mid = int(np.floor(255 * ((0.5 * (2.51 * 0.5 + 0.03)) / (0.5 * (2.43 * 0.5 + 0.59) + 0.14)) ** (1 / 2.2)))
    return [[mid, mid, 0], [255, 0, mid], [255, 255, 255], [0, 255, 255], [0, 0, 0], [255, 255, 255]]


# ------------------------------------------------------------------ the three copies of the curve under test


def _pack(fn, check, lead, rgb, tonemap, limit):
    import ctypes as C
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(lead) + [C.c_int32, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    rgb = np.ascontiguousarray(rgb, np.float32)
    out = np.full((len(rgb), 3), 77, np.uint8)
    check(fn(*lead, len(rgb), rgb.ctypes.data, int(tonemap), float(limit), out.ctypes.data))
    return out


def oracle_tone_pack(oracle, rgb, tonemap, limit):
    """jade_oracle_tone_pack: the statements the oracle's jade_render_resolve_ex runs."""
    return _pack(oracle.lib.jade_oracle_tone_pack, oracle.check, (), rgb, tonemap, limit)


def device_tone_pack(hip_debug, rgb, tonemap, limit):
    """jade_debug_tone_pack (libjade_hip_debug.so): tone_pack_bgr8 on device 0 - k_resolve's and k_dn_out's statements."""
    return _pack(hip_debug.lib.jade_debug_tone_pack, hip_debug.check, (0,), rgb, tonemap, limit)


def host_tone_pack(rgb, tonemap, limit):
    """jade_debug_tone_pack_host (libjade_hip_debug.so): the same tone_pack_bgr8 compiled for the host, what jade_render_multi packs
    the gathered frame with.  Makes no HIP call, so it runs without a GPU."""
    import ctypes as C
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = C.CDLL(path)

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"jade_debug_tone_pack_host: status {rc}")
    return _pack(lib.jade_debug_tone_pack_host, check, (), rgb, tonemap, limit)
