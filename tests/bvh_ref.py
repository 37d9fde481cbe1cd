"""The trees jade_bvh_build_lbvh and jade_bvh_build_ploc are meant to build, written from the statement in include/jade_bvh.h
("The tree, stated") and not from the kernels' form: plain numpy and Python, no GPU, no library of this project.

Every float the builders compute is a float32 sum, difference, product, quotient, minimum or maximum (the build contracts
nothing and divides correctly rounded), so numpy's float32 reproduces it to the bit and a tree is compared without a tolerance:
kinds, counts, offsets, box corners as uint32, the triangle order.  The section names in the comments are the header's."""
import numpy as np

F = np.float32
RADIUS = 16  # [PLOC] "within 16 positions"
DUMMY = (255, 128, 30, 0) + tuple(np.array([1, 1, 0, 0, 1, 0], F).view(np.uint32).tolist())  # [Records] node 0


# ------------------------------------------------------------------------------------------------------------ keys --
def _expand10(v):
    """10 bits -> every third bit (bit k of v to bit 3k)."""
    out = np.zeros(v.shape, np.uint64)
    for k in range(10):
        out |= ((v >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k)
    return out


def morton_keys(verts):
    """[Centroid and keys] verts (n, 3, 3) float32 -> the n keys, ascending."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        c = ((v[:, 0] + v[:, 1]) + v[:, 2]) / F(3)                      # ((p1 + p2) + p3) / 3
        cmin, cmax = c.min(0), c.max(0)
        ext = cmax - cmin
        scale = np.where(cmax > cmin, F(1023.999) / ext, F(0)).astype(F)  # 0 where the extent is not positive
        q = (c - cmin) * scale
    assert q.dtype == F
    q = np.where(q > 0, q, F(0))                                        # a NaN product goes to 0 ...
    q = np.where(q < 1023, q, F(1023)).astype(np.uint64)                # ... clamped to [0, 1023], truncated
    code = (_expand10(q[:, 0]) << np.uint64(2)) | (_expand10(q[:, 1]) << np.uint64(1)) | _expand10(q[:, 2])  # x highest
    keys = (code << np.uint64(32)) | np.arange(len(v), dtype=np.uint64)  # code << 32 | original index
    return np.sort(keys)


# ------------------------------------------------------------------------------------------------- binary trees ----
# A binary tree over the n sorted positions: items 0 .. n-1 are the triangles in key order, items n .. are internal with
# children (left[i - n], right[i - n]); `root` is the item at the top.


def lbvh_topology(keys):
    """[LBVH] top-down: a node over [a, b] splits after the last key that shares with key[a] more leading bits than key[b]."""
    n = len(keys)
    if n == 1:
        return [], [], 0
    k = [int(x) for x in keys]
    left, right = [], []

    def new():
        left.append(-1)
        right.append(-1)
        return n + len(left) - 1

    root = new()
    stack = [(root, 0, n - 1)]
    while stack:
        item, a, b = stack.pop()
        bit = (k[a] ^ k[b]).bit_length() - 1          # the highest bit in which the first and the last key differ
        first_right = ((k[a] >> bit) | 1) << bit      # the least key with key[a]'s prefix and a one there
        g = int(np.searchsorted(keys, np.uint64(first_right), side="left")) - 1
        assert a <= g < b
        for side, (lo, hi) in ((left, (a, g)), (right, (g + 1, b))):
            if lo == hi:
                side[item - n] = lo
            else:
                child = new()
                side[item - n] = child
                stack.append((child, lo, hi))
    return left, right, root


def union_area(lo_a, hi_a, lo_b, hi_b):
    """[PLOC] (x*y + y*z) + z*x of the union's extents, float32; a NaN (inf * 0) counts as +inf."""
    with np.errstate(all="ignore"):
        e = np.maximum(hi_a, hi_b) - np.minimum(lo_a, lo_b)
        x, y, z = e[..., 0], e[..., 1], e[..., 2]
        a = (x * y + y * z) + z * x
    assert a.dtype == F
    return np.where(np.isnan(a), F(np.inf), a)


def ploc_topology(keys, prim_lo, prim_hi):
    """[PLOC] rounds over arrays.  Returns (left, right, root, clusters at the start of every round)."""
    n = len(keys)
    prim = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    lo, hi = prim_lo[prim].copy(), prim_hi[prim].copy()
    cid = np.arange(n)
    left, right, sizes = [], [], []
    offs = np.array([d for d in range(-RADIUS, RADIUS + 1) if d != 0])
    while len(cid) > 1:
        m = len(cid)
        sizes.append(m)
        i = np.repeat(np.arange(m), len(offs))
        j = i + np.tile(offs, m)
        ok = (j >= 0) & (j < m)
        jc = np.clip(j, 0, m - 1)
        area = union_area(lo[i], hi[i], lo[jc], hi[jc])
        dist = np.abs(j - i)
        low = np.minimum(i, j)
        parity = (low // dist) & 1
        # the minimum per cluster of (area, distance, (low / distance) & 1, low); positions outside the row come last
        rank = np.lexsort((low, parity, dist, area, ~ok, i))
        best = rank[:: len(offs)]
        assert np.array_equal(i[best], np.arange(m)) and ok[best].all()
        nn = j[best]
        mutual = nn[nn] == np.arange(m)
        leader = mutual & (np.arange(m) < nn)          # the lower position keeps its place: the left child's side
        gone = mutual & (np.arange(m) > nn)
        assert leader.any(), "a PLOC round merged nothing"
        new_cid = cid.copy()
        for a in np.nonzero(leader)[0]:
            left.append(int(cid[a]))
            right.append(int(cid[nn[a]]))
            new_cid[a] = n + len(left) - 1
            lo[a] = np.minimum(lo[a], lo[nn[a]])
            hi[a] = np.maximum(hi[a], hi[nn[a]])
        keep = ~gone
        cid, lo, hi = new_cid[keep], lo[keep], hi[keep]
    return left, right, int(cid[0]), sizes


# ------------------------------------------------------------------------------------------- collapse and emit ----
class Binary:
    """A builder's binary tree with what every item needs for the records: count, first position in the triangle order, box."""

    def __init__(self, keys, prim_lo, prim_hi, left, right, root, rounds=None):
        n = len(keys)
        self.n, self.left, self.right, self.root, self.rounds = n, left, right, root, rounds
        prim = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        items = n + len(left)
        self.count = np.ones(items, np.int64)
        self.offset = np.zeros(items, np.int64)
        self.lo = np.zeros((items, 3), F)
        self.hi = np.zeros((items, 3), F)
        self.lo[:n], self.hi[:n] = prim_lo[prim], prim_hi[prim]
        # [Both builders] triangle order: depth-first, left before right
        dfs, post, stack = [], [], [root]
        while stack:
            it = stack.pop()
            post.append(it)
            if it < n:
                dfs.append(it)
            else:
                stack += [right[it - n], left[it - n]]
        assert sorted(dfs) == list(range(n))
        self.order = prim[dfs].astype(np.int32)
        pos = np.empty(n, np.int64)
        pos[dfs] = np.arange(n)
        self.offset[:n] = pos
        for it in reversed(post):                       # children before parents
            if it >= n:
                l, r = left[it - n], right[it - n]
                self.count[it] = self.count[l] + self.count[r]
                self.offset[it] = self.offset[l]
                assert self.offset[r] == self.offset[l] + self.count[l]
                self.lo[it] = np.minimum(self.lo[l], self.lo[r])
                self.hi[it] = np.maximum(self.hi[l], self.hi[r])

    def depth(self, leaf_size):
        d, stack = 0, [(self.root, 1)]
        while stack:
            it, k = stack.pop()
            d = max(d, k)
            if self.count[it] > leaf_size:
                stack += [(self.left[it - self.n], k + 1), (self.right[it - self.n], k + 1)]
        return d

    def emit(self, leaf_size):
        """[Both builders] a subtree of <= leaf_size triangles is one leaf.  (order, nodes[.., 10] uint32), root = 1, numbered in
        the order the walk below meets them (which number a node gets is not part of the contract)."""
        n = self.n
        recs = [list(DUMMY), None]
        stack = [(self.root, 1)]
        while stack:
            it, slot = stack.pop()
            box = np.concatenate([self.lo[it], self.hi[it]]).view(np.uint32).tolist()
            if self.count[it] <= leaf_size:
                recs[slot] = [0, 0, int(self.count[it]), int(self.offset[it])] + box
            else:
                l, r = len(recs), len(recs) + 1
                recs += [None, None]
                recs[slot] = [l, r, 0, 0] + box
                stack += [(self.left[it - n], l), (self.right[it - n], r)]
        return self.order.copy(), np.array(recs, np.uint32)


def binary(kind, verts):
    """The builder's tree before the collapse: depends on the triangles and the kind only, so cache it per input."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)
    assert np.isfinite(v).all(), "[Non-finite input] both builders refuse this"
    keys = morton_keys(v)
    prim_lo, prim_hi = v.min(1), v.max(1)
    if kind == "lbvh":
        left, right, root = lbvh_topology(keys)
        t = Binary(keys, prim_lo, prim_hi, left, right, root)
        assert np.array_equal(t.order, (keys & np.uint64(0xFFFFFFFF)).astype(np.int32))  # "for the LBVH it is the key order"
        return t
    assert kind == "ploc"
    left, right, root, sizes = ploc_topology(keys, prim_lo, prim_hi)
    return Binary(keys, prim_lo, prim_hi, left, right, root, rounds=sizes)


def build(kind, verts, leaf_size):
    """(order, nodes) in the form SceneBuilder.build_with_bvh takes."""
    return binary(kind, verts).emit(leaf_size)


# ------------------------------------------------------------------------------------------------- comparing ------
def tree_difference(a, b):
    """None if the trees (order, nodes) a and b are the same tree, else a line that names the first difference.  Walks both
    from node 1, left with left and right with right: kind, n, index, both box corners as bits; then the two orders."""
    (oa, na), (ob, nb) = a, b
    na = np.ascontiguousarray(na).view(np.uint32).reshape(-1, 10)
    nb = np.ascontiguousarray(nb).view(np.uint32).reshape(-1, 10)
    stack, visited = [(1, 1, "root")], 0
    while stack:
        ia, ib, path = stack.pop()
        if not (0 < ia < len(na) and 0 < ib < len(nb)):
            return f"{path}: node number out of range ({ia} of {len(na)}, {ib} of {len(nb)})"
        visited += 1
        if visited > len(na) + len(nb):
            return "a tree has a cycle"
        ra, rb = na[ia], nb[ib]
        if (ra[2] > 0) != (rb[2] > 0):
            return f"{path}: leaf against internal node ({ra[:4].tolist()} / {rb[:4].tolist()})"
        if not np.array_equal(ra[4:], rb[4:]):
            return f"{path}: boxes differ ({ra[4:].view(F).tolist()} / {rb[4:].view(F).tolist()})"
        if ra[2] > 0:
            if not np.array_equal(ra[:4], rb[:4]):
                return f"{path}: leaf records differ ({ra[:4].tolist()} / {rb[:4].tolist()})"
        else:
            if ra[2] != rb[2] or ra[3] != rb[3]:
                return f"{path}: n / index of an internal node differ ({ra[:4].tolist()} / {rb[:4].tolist()})"
            if 0 in (ra[0], ra[1], rb[0], rb[1]):
                return f"{path}: a child is missing ({ra[:4].tolist()} / {rb[:4].tolist()})"
            stack += [(int(ra[1]), int(rb[1]), path + "R"), (int(ra[0]), int(rb[0]), path + "L")]
    if visited != len(na) - 1 or visited != len(nb) - 1:
        return f"{visited} nodes reached, {len(na) - 1} and {len(nb) - 1} records given"
    if not np.array_equal(np.asarray(oa), np.asarray(ob)):
        w = np.nonzero(np.asarray(oa) != np.asarray(ob))[0]
        return f"orders differ at {len(w)} positions, first {w[0]}: {oa[w[0]]} / {ob[w[0]]}"
    return None


def same_tree(a, b):
    return tree_difference(a, b) is None


def check_invariants(hs, leaf_max=8):
    """A scene's tree is a valid tree: the dummy, every triangle in one leaf, leaf boxes and unions exact.  Returns the depth."""
    ni, nf, v = hs.node_i32(), hs.node_f32(), hs.vertices()
    nT = hs.n_triangles
    assert tuple(ni[0, :3]) == (255, 128, 30)
    seen = np.zeros(nT, np.int32)
    stack, depth = [(1, 1)], 0
    while stack:
        i, d = stack.pop()
        depth = max(depth, d)
        l, r, n, first = ni[i, :4]
        aa, bb = nf[i, 4:7], nf[i, 7:10]
        if n > 0:
            assert 1 <= n <= leaf_max and l == 0 and r == 0
            seen[first:first + n] += 1
            tv = v[first:first + n].reshape(-1, 3)
            assert np.array_equal(tv.min(0), aa) and np.array_equal(tv.max(0), bb)
        else:
            assert l > 0 and r > 0
            # parent box = union of the children's boxes, exactly
            assert np.array_equal(np.minimum(nf[l, 4:7], nf[r, 4:7]), aa) and np.array_equal(np.maximum(nf[l, 7:10], nf[r, 7:10]), bb)
            stack += [(l, d + 1), (r, d + 1)]
    assert (seen == 1).all() and depth == hs.bvh_depth < 127
    assert np.array_equal(np.sort(hs.a["mapping"]), np.arange(nT))
    return depth


# ---------------------------------------------------------------------------------------------------- inputs ------
LEAF_SIZES = (1, 3, 8, 15)
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)


def clustered(n, seed=None):
    """Small triangles: random centres in a 100 x 1 x 0.01 box, edges of 0.05."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    return (rng.random((n, 1, 3)) * np.array([100, 1, 0.01]) + rng.random((n, 3, 3)) * 0.05).astype(F)


def _strip(quads):
    k = np.arange(quads, dtype=F)[:, None, None] * np.array([1, 0, 0], F)
    lower = TRI[None] + k
    upper = np.array([[1, 0, 0], [1, 1, 0], [0, 1, 0]], F)[None] + k
    return np.stack([lower, upper], 1).reshape(-1, 3, 3)


def _grid(nx, ny):
    cell = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), [0], indexing="ij"), -1).reshape(-1, 1, 1, 3).astype(F)
    two = np.stack([TRI, np.array([[1, 0, 0], [1, 1, 0], [0, 1, 0]], F)])[None]
    return (cell + two).reshape(-1, 3, 3)


def _make_inputs():
    d = {}
    # sizes: n = 1 (no radix tree) and 2; fewer clusters than one search radius and exactly 2 * 16 + 1; one block of 256, +- 1;
    # one block and its 16-box halo, + 1; several blocks, the cluster count crossing 512 and 256 again in later rounds
    for n in (1, 2, 3, 17, 33, 255, 256, 257, 272, 273, 600, 1500):
        d[f"clustered{n}"] = clustered(n)
    # one Morton code for all (the LBVH splits on the index bits of the key only, PLOC is all ties)
    d["duplicates300"] = np.tile(TRI[None], (300, 1, 1))
    d["instanced50x8"] = np.tile(np.random.default_rng(3).random((50, 3, 3)).astype(F), (8, 1, 1))
    # exact area ties, z extent zero (the scale is 0 on an axis)
    d["strip600"] = _strip(300)
    d["grid20x20"] = _grid(20, 20)
    # quantisation edges
    rng = np.random.default_rng(7)
    v = (rng.random((120, 1, 3)) * 4 + rng.random((120, 3, 3)) * 0.1).astype(F)
    v[77] = np.array([9, 9, 9], F) + TRI * F(0.1)                      # alone at cmax on every axis: the product exceeds 1023
    d["alone_at_cmax"] = v
    v = (rng.random((200, 3, 3)) * 0.9 + rng.permutation(200)[:, None, None] * np.array([1, 0, 0])).astype(F)  # no two overlap
    v[:, :, 1] = np.where(rng.random(200) < 0.5, F(0), F(1e-42))[:, None]  # y extent a denormal: the scale is inf, 0 * inf occurs
    d["denormal_y"] = v
    v = np.concatenate([clustered(150, seed=9) * F(0.01), clustered(150, seed=10) * F(0.01) + np.array([50, 0, 0], F), (TRI + F(1e6))[None]])
    d["outlier"] = v.astype(F)                                         # most triangles in a handful of codes
    # large magnitudes
    rng = np.random.default_rng(11)
    d["huge_all_inf"] = (rng.random((300, 1, 3)) * 1e19 + rng.random((300, 3, 3)) * 3e19).astype(F)   # every union area overflows
    d["huge_mixed"] = (rng.random((300, 1, 3)) * 3e19 + rng.random((300, 3, 3)) * 1e18).astype(F)     # some do, some do not
    d["clustered600_x2^40"] = clustered(600) * F(2.0 ** 40)
    d["clustered600_x2^-40"] = clustered(600) * F(2.0 ** -40)
    # extents that overflow beside a flat axis: inf * 0, a NaN area, which counts as +inf.  (p1 + p2) + p3 stays finite.
    a = (rng.random((64, 3)) * 1e38 + 2e38).astype(F)
    a[:, 2] = 0
    c = ((rng.random((64, 3)) - 0.5) * 2e38).astype(F)
    c[:, 2] = 0
    d["nan_area"] = np.stack([a, -a, c], 1) + F(0)                    # + 0: no -0.0, which a scene's transform does not keep
    for k, v in d.items():
        assert v.dtype == F and v.shape[1:] == (3, 3) and np.isfinite(v).all(), k
    return d


_inputs = None
_binaries = {}


def inputs():
    """{name: (n, 3, 3) float32 vertices}: the smallest shapes at which the builders' kernels can go wrong.  Fixed seeds."""
    global _inputs
    if _inputs is None:
        _inputs = _make_inputs()
    return _inputs


def binary_of(name, kind):
    """The stated binary tree of a named input, built once per (input, kind)."""
    if (name, kind) not in _binaries:
        _binaries[(name, kind)] = binary(kind, inputs()[name])
    return _binaries[(name, kind)]


def reference(name, kind, leaf_size, verts=None):
    """The stated tree (order, nodes) of a named input.  `verts`: the vertices as the builder under test is given them - they
    must be the input's own bits."""
    if verts is not None:
        v = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)
        assert np.array_equal(v.view(np.uint32), inputs()[name].view(np.uint32))
    return binary_of(name, kind).emit(leaf_size)
