"""The frames, variances and parameters on which the despeckle pass is held to its float32 statement bit for bit
(tests/test_despeckle_cpu.py without a GPU, tests/test_gpu_despeckle_exact.py on the device).  Frames are float32 [H, W, 3] and
variances float32 [H, W], seeded by kind and shape, read-only and made once; so is the statement's result for a case (`want`).

Shapes are written W x H and straddle k_despeckle's block of 32 x 8 pixels and its halo of R <= 3: one pixel, less than a halo,
less than a block, one column / one row more than a block, and many blocks down a frame narrower than a halo."""
import functools
import typing
import zlib

import numpy as np

import despeckle_spec as S

F32_MAX = float(np.float32(3.4028235e38))
SHAPES = ((1, 1), (3, 2), (24, 17), (33, 20), (40, 7), (3, 257))  # (W, H)
TALL = (1, 8 * 65535)  # 1 x 524280, the height limit: 65535 blocks in grid.y of k_despeckle
KINDS = ("decades", "speckles", "clusters", "constant", "ties", "zeros", "negative", "bad", "top", "extremes")
VARIANCES = ("none", "nan", "negative", "tiny", "huge", "sampled", "flow")
BAD_BITS = (0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000)  # NaNs quiet, negative and signalling; +inf; -inf


def _ground(rng, h, w, level=0.2):
    """a smooth, slightly noisy ground"""
    return (level * (0.75 + 0.5 * rng.random((h, w, 3)))).astype(np.float32)


def _decades(rng, h, w):
    """colours over six decades: every pixel is somebody's speckle"""
    return (rng.random((h, w, 3)) * 10.0 ** rng.uniform(-3, 3, (h, w, 1))).astype(np.float32)


def _plant(rng, x, n, size):
    """n bright runs of `size` = (rows, columns) pixels, 1e2 .. 1e4 times the ground, borders and corners included"""
    h, w = x.shape[:2]
    spots = [(0, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0)] + [(int(rng.integers(h)), int(rng.integers(w))) for _ in range(n)]
    ground = x.copy()
    for y, xx in spots:
        x[y:y + size[0], xx:xx + size[1]] = ground[y, xx] * np.float32(10.0 ** rng.uniform(2, 4))
    return x


def _speckles(rng, h, w):
    """planted single speckles"""
    return _plant(rng, _ground(rng, h, w), max(3, h * w // 40), (1, 1))


def _clusters(rng, h, w):
    """adjacent pairs (both directions) and 2 x 2 clusters: what rank and iterations are for"""
    x = _ground(rng, h, w)
    for size in ((1, 2), (2, 1), (2, 2)):
        x = _plant(rng, x, max(2, h * w // 120), size)
    return x


def _constant(rng, h, w):
    return np.full((h, w, 3), 0.7, np.float32)


def _ties(rng, h, w):
    """three levels only, so the K-th largest falls among exact ties; the top level is above twice the middle one"""
    lv = np.float32([0.125, 0.5, 4.0])[rng.choice(3, (h, w), p=(0.5, 0.35, 0.15))]
    return np.repeat(lv[..., None], 3, -1).astype(np.float32)


def _zeros(rng, h, w):
    """zeros of either sign with a few positive pixels among them: B = +-0, C = floor"""
    x = np.where(rng.random((h, w, 3)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    lit = rng.random((h, w)) < 0.12
    x[lit] = (rng.random((int(lit.sum()), 3)) * 3.0).astype(np.float32)
    return x


def _negative(rng, h, w):
    """channels of either sign: Y negative, zero by cancellation, or positive with a negative channel"""
    return (rng.normal(size=(h, w, 3)) * 10.0 ** rng.uniform(-2, 2, (h, w, 1))).astype(np.float32)


def _bad(rng, h, w):
    """NaN and +-inf pixels alone and right next to speckles"""
    x = _speckles(rng, h, w)
    bits = x.view(np.uint32)
    y = S.luminance(x)
    ys, xs = np.nonzero(y > 5.0)
    spots = [(0, 0, 0), (h - 1, w - 1, 2), (h // 2, w // 2, 1)]
    spots += [(min(int(a) + 1, h - 1), int(b), i % 3) for i, (a, b) in enumerate(zip(ys[::2], xs[::2]))]  # under every other speckle
    spots += [(int(a), max(int(b) - 1, 0), i % 3) for i, (a, b) in enumerate(zip(ys[1::3], xs[1::3]))]      # left of some
    for i, (yy, xx, ch) in enumerate(spots):
        if h * w > 1 or i == 0:
            bits[yy, xx, ch] = BAD_BITS[i % len(BAD_BITS)]
    return x


def _top(rng, h, w):
    """channels near the largest float: Y = 0.3 r + 0.6 g + 0.1 b stays finite for most and overflows where r and g are both at the top"""
    x = (rng.random((h, w, 3)) ** 0.125 * F32_MAX).astype(np.float32)
    x = np.minimum(x, np.float32(F32_MAX))
    x[rng.random((h, w)) < 0.3] *= np.float32(1e-3)
    x[rng.random((h, w)) < 0.1] = np.float32(F32_MAX)
    return x


def _extremes(rng, h, w):
    """the left half 1e-30 with speckles 1e8 times that (d * d underflows), the right half 1e15 with speckles 1e10 times that (d * d
    overflows)"""
    x = _ground(rng, h, w, 1.0)
    x = _plant(rng, x, max(3, h * w // 30), (1, 1))
    y = S.luminance(x)
    left = np.arange(w)[None, :] < (w + 1) // 2
    lit = y > 5.0
    scale = np.where(left, np.where(lit, 1e-26, 1e-30), np.where(lit, 1e21, 1e15))
    return (x * scale[..., None]).astype(np.float32)


_MAKE = dict(decades=_decades, speckles=_speckles, clusters=_clusters, constant=_constant, ties=_ties, zeros=_zeros, negative=_negative,
             bad=_bad, top=_top, extremes=_extremes)


@functools.lru_cache(maxsize=None)
def frame(kind, w, h):
    """The frame of this kind at W x H: float32 [H, W, 3], read-only."""
    rng = np.random.default_rng([zlib.crc32(kind.encode()), w, h])
    x = np.ascontiguousarray(_MAKE[kind](rng, h, w), np.float32)
    assert x.shape == (h, w, 3)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def variance(vkind, kind, w, h):
    """The variance of this kind for that frame: float32 [H, W], read-only; None for "none".  Never +-inf and no NaN but the plain quiet
    one: (k * k) * v then makes no NaN of its own, whose bits the statement does not fix."""
    if vkind == "none":
        return None
    rng = np.random.default_rng([zlib.crc32(vkind.encode()), zlib.crc32(kind.encode()), w, h])
    with np.errstate(all="ignore"):
        y = np.nan_to_num(S.luminance(frame(kind, w, h)).astype(np.float64), nan=1.0, posinf=1e30, neginf=-1e30)
        if vkind == "nan":
            v = np.full((h, w), np.nan)
        elif vkind == "negative":  # negative entries (and -0.0) among sampled ones
            v = y * y * 10.0 ** rng.uniform(-3, 1, (h, w))
            v = np.where(rng.random((h, w)) < 0.4, -v, v)
            v[rng.random((h, w)) < 0.1] = -0.0
        elif vkind == "tiny":      # every excess is established
            v = np.minimum(y * y * 1e-12, 1e30)
        elif vkind == "huge":      # none is
            v = np.full((h, w), 1e38)
        elif vkind == "sampled":   # the standard error between a thirtieth of the pixel and three times it: some are, some are not
            v = np.minimum(y * y * 10.0 ** rng.uniform(-3, 1, (h, w)), 1e30)
        else:                      # "flow": zz * v underflows (denormal v), overflows (v near the top), or is 0
            v = rng.choice([1.4e-45, 1e-41, 3e38, 1e38, 0.0, 1e-20, 1e20], (h, w))
        v = np.ascontiguousarray(np.clip(v, -3e38, 3e38), np.float32)  # (clip passes a NaN through)
    assert v.shape == (h, w) and not np.isinf(v).any()
    v.setflags(write=False)
    return v


class Case(typing.NamedTuple):
    kind: str
    vkind: str
    w: int
    h: int
    iterations: int
    radius: int
    rank: int
    gain: float
    floor: float
    sigmas: float

    @property
    def id(self):
        return (f"{self.kind}-{self.vkind}-{self.w}x{self.h}-i{self.iterations}-R{self.radius}-K{self.rank}-g{self.gain:g}-f{self.floor:g}"
                f"-z{self.sigmas:g}")

    @property
    def params(self):
        return dict(iterations=self.iterations, radius=self.radius, rank=self.rank, gain=self.gain, floor=self.floor, sigmas=self.sigmas)


def _cases():
    out = []

    def add(kind, vkind, wh, iterations=1, radius=1, rank=2, gain=2.0, floor=0.0, sigmas=2.0):
        c = Case(kind, vkind, wh[0], wh[1], iterations, radius, rank, float(np.float32(gain)), float(np.float32(floor)), float(np.float32(sigmas)))
        if c not in out:
            out.append(c)

    for n, wh in enumerate(SHAPES):  # every shape at every radius and rank (a corner's three neighbours cannot reach rank 4)
        for radius in (1, 2, 3):
            for rank in (1, 2, 3, 4):
                kind = ("speckles", "clusters", "decades")[(n + radius + rank) % 3]
                vkind = ("none", "sampled")[(radius + rank) % 2]
                add(kind, vkind, wh, 1 + (n + rank) % 2, radius, rank)
    for wh in ((24, 17), (33, 20)):  # every number of passes, where rank 1 needs them: a pair is peeled one pixel per pass at best
        for iterations in (1, 2, 3, 4):
            add("clusters", "none", wh, iterations, 1, 1)
            add("clusters", "sampled", wh, iterations, 2, 3, 1.5)
            add("decades", "sampled", wh, iterations, 1, 2, 1.0, 0.0, 3.0)
    for wh in ((40, 7), (33, 20)):  # every kind of frame under every kind of variance
        for kind in KINDS:
            for vkind in VARIANCES:
                add(kind, vkind, wh)
            add(kind, "sampled", wh, 2, 2, 3, 4.0, 0.25, 1.0)
            add(kind, "sampled", wh, 1, 3, 4, 1.0, 1e-3, 0.0)
    for gain in (1.0, 1.5, 2.0, 4.0):  # the parameters' ranges, the floor against the zeros
        add("speckles", "sampled", (33, 20), 1, 1, 2, gain)
        add("zeros", "none", (33, 20), 1, 1, 2, gain, 0.5)
        add("zeros", "none", (24, 17), 2, 2, 1, gain, -0.0)
    for sigmas in (0.0, 1.0, 4.0, 1e19, 1e-30):  # z * z fine, overflowing to inf and underflowing to 0
        add("speckles", "sampled", (24, 17), 1, 1, 2, 2.0, 0.0, sigmas)
        add("extremes", "flow", (33, 20), 1, 1, 2, 2.0, 0.0, sigmas)
    return out


CASES = _cases()
TALL_CASE = Case("speckles", "sampled", TALL[0], TALL[1], 2, 3, 2, 2.0, 0.0, 2.0)
IN_PLACE_CASE = Case("clusters", "sampled", 33, 20, 2, 2, 2, 2.0, 0.0, 2.0)


@functools.lru_cache(maxsize=None)
def want(case, variant=None):
    """The float32 statement's (colour, variance | None, scale, report) for this case, arrays read-only."""
    c, v, s, rep = S.despeckle(frame(case.kind, case.w, case.h), variance(case.vkind, case.kind, case.w, case.h), variant=variant, **case.params)
    for a in (c, v, s):
        if a is not None:
            assert a.dtype == np.float32
            a.setflags(write=False)
    return c, v, s, rep


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want_):
    """whether two results (colour, variance | None, scale, report) agree in every bit and every count"""
    for g, w in zip(got[:3], want_[:3]):
        if (g is None) != (w is None) or (g is not None and not np.array_equal(bits(g), bits(w))):
            return False
    return dict(got[3]) == dict(want_[3])


def differences(got, want_, limit=6):
    """what differs, for a failure's message: per output the count of differing words and the first few (index, got, want) in hex"""
    out = {}
    for name, g, w in zip(("rgb", "variance", "scale"), got[:3], want_[:3]):
        if g is None or w is None:
            if (g is None) != (w is None):
                out[name] = "one is missing"
            continue
        gb, wb = bits(g).ravel(), bits(w).ravel()
        idx = np.nonzero(gb != wb)[0]
        if len(idx):
            out[name] = (int(len(idx)), [(int(i), f"{gb[i]:08x}", f"{wb[i]:08x}") for i in idx[:limit]])
    if dict(got[3]) != dict(want_[3]):
        out["report"] = (dict(got[3]), dict(want_[3]))
    return out
