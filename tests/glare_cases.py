"""The frames and parameters on which glare is held to its float32 statement bit for bit (tests/test_glare_cpu.py without a GPU,
tests/test_gpu_glare_exact.py on the device).  Frames are float32 [H, W, 3], seeded by kind and shape, read-only and made once; so
is the statement's result for a case (`want`).

Shapes are written W x H, each named for what it straddles: a k_gl_reduce block makes 32 x 8 outputs from 67 x 19 sources,
k_gl_expand_add and k_gl_out blocks are 16 x 16."""
import functools
import typing
import zlib

import numpy as np

import glare_ref as G

F32_MAX = float(np.float32(3.4028235e38))
TINY = float(np.nextafter(np.float32(0), np.float32(1)))  # 1.4e-45, the smallest positive float

KINDS = ("decades", "halo", "signed", "denormal", "top", "constant", "bad")
SHAPES = {  # name -> (W, H)
    "1x1": (1, 1), "2x1": (2, 1), "1x2": (1, 2), "3x3": (3, 3),
    "67x1 one source row": (67, 1), "1x67 one source column": (1, 67),
    "64x16 exactly one reduce block": (64, 16),
    "65x17 a second block of one column and one row": (65, 17),
    "131x35 three blocks across": (131, 35),
    "33x33": (33, 33),
    "45x27 the render's": (45, 27),
    "131x67": (131, 67),
}
TALL = (1, 16 * 65535)  # 1 x 1048560, the height limit: 65535 blocks in grid.y of k_gl_out and of k_gl_reduce's level 1
LEVELS = (1, 2, 6, 12)
FALLOFFS = (0.5, 1.0, 2.0, 0.05, 1e30, 1e-30, F32_MAX, TINY)
# The caller's doubles; the library (and the statement) round them to float.  0.6 is beyond the three that were asked for: of those,
# none tells 1 - s as one float subtraction from 1 - s taken in double and rounded (tests/test_glare_cpu.py's break table); 0.6 does.
STRENGTHS = (TINY, 0.3, 1.0, 0.6)
SWEEP = ((65, 17), (33, 33))        # every falloff and every strength
ALL_KINDS = ((65, 17), (131, 35))   # every kind of frame

BAD_BITS = {"nan": (0x7fc00001, 0xffc12345, 0x7f800001), "+inf": 0x7f800000, "-inf": 0xff800000}  # quiet, negative, signalling


def _decades(rng, h, w):
    """colours over six decades (tests/test_gpu_glare.py's frames)"""
    return (rng.random((h, w, 3)) * 10.0 ** rng.uniform(-3, 3, (h, w, 1))).astype(np.float32)


def _halo(rng, h, w):
    """what glare is for: a bright 8 x 8 centre (about 1e3) on a dim ground (about 1e-3), and where the frame has room a second
    bright block touching the upper left corner"""
    x = 1e-3 * (0.5 + rng.random((h, w, 3)))
    y0, x0 = max(h // 2 - 4, 0), max(w // 2 - 4, 0)
    x[y0:y0 + 8, x0:x0 + 8] = 1e3 * (0.5 + rng.random(x[y0:y0 + 8, x0:x0 + 8].shape))
    if w >= 24 and h >= 12:
        x[:6, :5] = 1e3 * (0.5 + rng.random((6, 5, 3)))
    return x.astype(np.float32)


def _signed(rng, h, w):
    """mixed signs with runs of -0.0: 12 x 12 at the upper left corner, 7 rows along the lower border, 9 x 9 inside - wide enough that
    whole filter neighbourhoods are -0.0, whose sum is -0.0 only if it does not start at +0"""
    x = (rng.normal(size=(h, w, 3)) * 10.0 ** rng.uniform(-2, 2, (h, w, 1))).astype(np.float32)
    x[:12, :12] = -0.0
    x[max(h - 7, 0):, w // 3:w // 3 + 20] = -0.0
    x[h // 2 - 2:h // 2 + 7, (2 * w) // 3:(2 * w) // 3 + 9] = -0.0
    x[:, w - 1:][:5] = 0.0  # a few +0.0 against them at the right border
    return x


def _denormal(rng, h, w):
    """1e-45 .. 1.2e-38 with either sign: every value is denormal or just above, so the products by 1/16 and 1/8 are denormal or
    underflow"""
    mag = np.maximum(10.0 ** rng.uniform(-45.0, np.log10(1.2e-38), (h, w, 3)), TINY)
    return (mag * rng.choice([-1.0, 1.0], (h, w, 3))).astype(np.float32)


def _top(rng, h, w):
    """non-negative values up to the largest float, so that no inf - inf can arise; a run of the largest itself at the upper border"""
    x = (rng.random((h, w, 3)) ** 0.25 * F32_MAX).astype(np.float32)
    x[rng.random((h, w)) < 0.1] = 0.0
    x[:3, w // 4:w // 4 + 9] = F32_MAX
    return np.minimum(x, np.float32(F32_MAX))


def _constant(rng, h, w):
    return np.full((h, w, 3), 0.7, np.float32)


def bad_pixels(h, w):
    """[(y, x, channel, bits)]: a corner, an edge and the interior"""
    nan = BAD_BITS["nan"]
    return [(0, 0, 0, BAD_BITS["+inf"]), (h - 1, w - 1, 2, BAD_BITS["-inf"]), (h // 2, 0, 1, nan[0]), (0, w // 2, 0, nan[1]),
            (h // 3, w // 3, 2, nan[2]), ((2 * h) // 3, w // 2, 1, BAD_BITS["-inf"]), ((2 * h) // 3, w // 2, 2, nan[0] + 6)]


def _bad(rng, h, w):
    x = _decades(rng, h, w)
    bits = x.view(np.uint32)
    for y, xx, c, b in bad_pixels(h, w):
        bits[y, xx, c] = b
    return x


_MAKE = dict(decades=_decades, halo=_halo, signed=_signed, denormal=_denormal, top=_top, constant=_constant, bad=_bad)


@functools.lru_cache(maxsize=None)
def frame(kind, w, h):
    """The frame of this kind at W x H: float32 [H, W, 3], read-only."""
    rng = np.random.default_rng([zlib.crc32(kind.encode()), w, h])
    x = np.ascontiguousarray(_MAKE[kind](rng, h, w), np.float32)
    assert x.shape == (h, w, 3)
    x.setflags(write=False)
    return x


def bad_mask(x):
    return ~np.isfinite(x).all(-1)


class Case(typing.NamedTuple):
    kind: str
    w: int
    h: int
    levels: int
    falloff: float   # a float32 value, as the library receives it
    strength: float  # the caller's double

    @property
    def id(self):
        return f"{self.kind}-{self.w}x{self.h}-L{self.levels}-f{self.falloff:.3g}-s{self.strength:.3g}"


def _levels_for(w, h, i):
    """every shape sees two of the four level counts, the small ones 12: far more than they have pixels for"""
    if w * h <= 9:
        return (12, 1, 2, 6)[i % 4]
    return LEVELS[(w + h + i) % 4]


def _cases():
    out = []

    def add(kind, wh, levels, falloff, strength):
        c = Case(kind, wh[0], wh[1], levels, float(np.float32(falloff)), float(strength))
        if c not in out:
            out.append(c)

    for n, wh in enumerate(SHAPES.values()):  # every shape with decades and halo at 0.5 and 2.0
        for i, (kind, f) in enumerate((("decades", 0.5), ("halo", 2.0), ("halo", 0.5), ("decades", 2.0))):
            add(kind, wh, _levels_for(*wh, n + i), f, 0.3)
    for wh, levels in zip(SWEEP, (12, 6)):  # every falloff and every strength
        for f in FALLOFFS:
            add("decades", wh, levels, f, 0.3)
            add("halo", wh, 2, f, 1.0)
        for s in STRENGTHS:
            add("halo", wh, levels, 0.5, s)
            add("decades", wh, 6, 2.0, s)
            add("signed", wh, 2, 1.0, s)
    for wh in ALL_KINDS:  # every kind of frame
        for kind in KINDS:
            add(kind, wh, 6, 0.5, 0.3)
            add(kind, wh, 12, 2.0, 1.0)
            add(kind, wh, 1, 1.0, TINY)
    return out


CASES = _cases()
TALL_CASE = Case("decades", TALL[0], TALL[1], 12, 0.5, 0.3)
# EXPAND(REDUCE(c)) alone, and with one expand_add: levels 1 and 2 at strength 1 (the weights of one level are 1, and 1 - s is 0)
OPERATOR_FRAMES = [(kind, w, h) for (w, h) in ((1, 1), (3, 3), (65, 17), (131, 35), (33, 33)) for kind in KINDS]


def operator_case(kind, w, h, levels):
    return Case(kind, w, h, levels, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def want(case):
    """The float32 statement's frame for this case, read-only."""
    with np.errstate(all="ignore"):
        out = G.glare(frame(case.kind, case.w, case.h), case.levels, case.strength, case.falloff, np.float32)
    assert out.dtype == np.float32
    out.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differences(got, want_, limit=8):
    """(count of differing pixels, the first few as (x, y, got bits, want bits)) - bits as three hex words per pixel"""
    g, w = bits(got), bits(want_)
    diff = (g != w).any(-1)
    ys, xs = np.nonzero(diff)
    first = [(int(x), int(y), tuple(f"{v:08x}" for v in g[y, x]), tuple(f"{v:08x}" for v in w[y, x])) for y, x in zip(ys[:limit], xs[:limit])]
    return int(diff.sum()), first
