"""tests/bvh_ref.py, the stated trees of include/jade_bvh.h, checked on its own before the device is compared with it
(tests/test_gpu_bvh_exact.py): on every input and for both builders the reference's tree is a valid tree, shallow enough for the
traversal stack, and the oracle finds through it exactly what it finds in a flat scan; PLOC's rounds all merge; and the smallest
trees are written down by hand."""
import numpy as np
import pytest

import bvh_ref as R
from conftest import J

NAMES = list(R.inputs())
# the reference's "no hit" distance is 2^31 - 1 (PathTrace.cu:23) and a hit beyond it is a miss: the rays below start a few
# triangle sizes from their target, which in these sets is 10^11 or more.  The walk is compared all the same; no hit is asked for.
NO_HITS_EXPECTED = {"huge_all_inf", "huge_mixed", "nan_area", "clustered600_x2^40"}

_scenes = {}


def _scene(name):
    """(builder, the vertices as the builders read them, the flat scene's answers to 2000 rays) - once per input."""
    if name not in _scenes:
        from jaderaytracerendering_amd import host as H
        v = R.inputs()[name]
        b = J.SceneBuilder()
        b.add_mesh(v.reshape(-1, 3), np.arange(3 * len(v)).reshape(-1, 3), H.material())
        b.set_env_sky(16, 8)
        got = b.triangles_original().view(np.float32)[:, 1:10].reshape(-1, 3, 3)
        assert np.array_equal(got.view(np.uint32), v.view(np.uint32))     # the builder hands on the input's bits
        rng = np.random.default_rng(2)
        n = 2000
        v64 = v.astype(np.float64)
        t = rng.integers(0, len(v), n)
        w = rng.dirichlet((1, 1, 1), n)
        target = (v64[t] * w[:, :, None]).sum(1)                           # a point of a random triangle ...
        size = np.minimum(np.ptp(v64[t], axis=1).max(1), 1e36)[:, None]
        away = rng.normal(size=(n, 3))
        away /= np.linalg.norm(away, axis=1, keepdims=True)
        o = (target + away * size * rng.uniform(2, 20, (n, 1))).astype(np.float32)  # ... seen from a few of its sizes away
        d = (-away).astype(np.float32)
        _scenes[name] = (b, got, (o, d, np.full(n, -1, np.int32)), {})
    return _scenes[name]


def _flat_answers(oracle, name):
    b, _, rays, cache = _scene(name)
    if "flat" not in cache:
        flat = b.build(10 ** 9)
        with oracle.scene(flat) as sf:
            i_f, d_f, _, _ = sf.trace_rays(*rays)
        cache["flat"] = (flat.vertices(), i_f, d_f)
    return cache["flat"]


@pytest.mark.parametrize("kind", ["lbvh", "ploc"])
@pytest.mark.parametrize("name", NAMES)
def test_reference_tree_is_valid_shallow_and_traces_like_a_flat_scan(oracle, name, kind):
    b, verts, rays, _ = _scene(name)
    fv, i_f, d_f = _flat_answers(oracle, name)
    for leaf_size in R.LEAF_SIZES:
        order, nodes = R.reference(name, kind, leaf_size, verts)
        hs = b.build_with_bvh(order, nodes)
        depth = R.check_invariants(hs, leaf_max=leaf_size)
        assert depth == R.binary_of(name, kind).depth(leaf_size) < 64
        with oracle.scene(hs) as st:
            it, dt, _, _ = st.trace_rays(*rays)
        h = it >= 0
        assert np.array_equal(h, i_f >= 0)
        assert name in NO_HITS_EXPECTED or h.sum() > 200
        assert np.array_equal(dt[h].view(np.uint32), d_f[h].view(np.uint32))      # same distance as a full scan
        assert np.array_equal(hs.vertices()[it[h]], fv[i_f[h]])                   # ... on the same triangle


@pytest.mark.parametrize("name", NAMES)
def test_every_ploc_round_of_the_reference_merges(name):
    """ploc_topology asserts it round by round; here also that the rounds are the few tens a row of ties must not exceed."""
    rounds = R.binary_of(name, "ploc").rounds
    n = len(R.inputs()[name])
    assert rounds == sorted(rounds, reverse=True) and len(set(rounds)) == len(rounds)
    assert (rounds[0] if rounds else 1) == n and len(rounds) <= 64


def test_same_tree_tells_trees_apart():
    a = R.reference("clustered33", "ploc", 3)
    b = R.reference("clustered33", "lbvh", 3)
    assert R.same_tree(a, a) and R.same_tree(b, (b[0].copy(), b[1].copy())) and not R.same_tree(a, b)
    order, nodes = b
    # renumbering is not a difference: reverse the records behind the root
    perm = np.concatenate([[0, 1], np.arange(len(nodes) - 1, 1, -1)])
    inv = np.argsort(perm)
    moved = nodes[perm].copy()
    inner = moved[:, 2] == 0
    inner[0] = False
    moved[inner, 0], moved[inner, 1] = inv[moved[inner, 0]], inv[moved[inner, 1]]
    assert R.same_tree(b, (order, moved))
    # one bit of one box corner, children swapped, a leaf's offset, two entries of the order
    for col, row in ((9, len(nodes) - 1), (4, 1)):
        x = nodes.copy()
        x[row, col] ^= 1
        assert not R.same_tree(b, (order, x))
    x = nodes.copy()
    x[1, 0], x[1, 1] = nodes[1, 1], nodes[1, 0]
    assert not R.same_tree(b, (order, x))
    leaf = np.nonzero(nodes[1:, 2] > 0)[0][0] + 1
    x = nodes.copy()
    x[leaf, 3] += 1
    assert not R.same_tree(b, (order, x))
    o2 = order.copy()
    o2[[0, 1]] = o2[[1, 0]]
    assert not R.same_tree(b, (o2, nodes))


# ------------------------------------------------------------------------------------------------- by hand --------
def _row(spans):
    """Triangles (x0, 0, 0), (x1, 0, 0), (x0, 1, 0): y extent 1, z extent 0, so the area of a union is its x extent and the
    Morton code holds the x bits only; centroid x = x0 + (x1 - x0) / 3."""
    return np.array([[[x0, 0, 0], [x1, 0, 0], [x0, 1, 0]] for x0, x1 in spans], np.float32)


def _nested(order, nodes, i=1):
    """A tree as nested tuples: a leaf is the tuple of its triangles' original indices, in order."""
    l, r, n, first = (int(x) for x in nodes[i, :4])
    if n > 0:
        return tuple(int(x) for x in order[first:first + n])
    return (_nested(order, nodes, l), _nested(order, nodes, r))


def _box(nodes, i):
    return nodes[i, 4:].view(np.float32).tolist()


def test_two_triangles_by_hand():
    """Given as (x = 5, x = 0): the key order is (1, 0), one root over two leaves, the lower key on the left - either builder."""
    v = _row([(5, 6), (0, 1)])
    for kind in ("lbvh", "ploc"):
        order, nodes = R.build(kind, v, 1)
        assert order.tolist() == [1, 0] and len(nodes) == 4
        assert _nested(order, nodes) == ((1,), (0,))
        l, r = int(nodes[1, 0]), int(nodes[1, 1])
        assert nodes[1, 2:4].tolist() == [0, 0] and nodes[l, :4].tolist() == [0, 0, 1, 0] and nodes[r, :4].tolist() == [0, 0, 1, 1]
        assert _box(nodes, 1) == [0, 0, 0, 6, 1, 0] and _box(nodes, l) == [0, 0, 0, 1, 1, 0] and _box(nodes, r) == [5, 0, 0, 6, 1, 0]
        assert nodes[0].tolist() == list(R.DUMMY)
        for leaf_size in (2, 15):
            order, nodes = R.build(kind, v, leaf_size)
            assert order.tolist() == [1, 0] and nodes[1].tolist() == [0, 0, 2, 0] + np.array([0, 0, 0, 6, 1, 0], np.float32).view(np.uint32).tolist()


def test_three_triangles_by_hand():
    """A = [0, 1], B = [1.5, 4.5], C = [4.625, 5.625], given as (C, A, B).  Centroids 1/3, 2.5, 4.958: quantised over an extent of
    4.625 to 0, 479, 1023, and only C has the top x bit, so the LBVH is ((A, B), C).  PLOC: A u B is 4.5 wide, B u C 4.125, A u C
    5.625; B and C choose each other, A (whose best is B) waits, then joins from the lower position: (A, (B, C))."""
    v = _row([(4.625, 5.625), (0, 1), (1.5, 4.5)])
    order, nodes = R.build("lbvh", v, 1)
    assert order.tolist() == [1, 2, 0] and _nested(order, nodes) == (((1,), (2,)), (0,))
    assert _box(nodes, 1) == [0, 0, 0, 5.625, 1, 0] and _box(nodes, int(nodes[1, 0])) == [0, 0, 0, 4.5, 1, 0]
    order, nodes = R.build("ploc", v, 1)
    assert order.tolist() == [1, 2, 0] and _nested(order, nodes) == ((1,), ((2,), (0,)))
    assert _box(nodes, int(nodes[1, 1])) == [1.5, 0, 0, 5.625, 1, 0]
    assert _nested(*R.build("lbvh", v, 2)) == ((1, 2), (0,)) and _nested(*R.build("ploc", v, 2)) == ((1,), (2, 0))
    assert _nested(*R.build("lbvh", v, 3)) == (1, 2, 0) == _nested(*R.build("ploc", v, 3))


def test_four_triangles_by_hand():
    """Unit-wide triangles at x = 0, 4.75, 5.25, 10.25 (A, B, C, D), given as (C, D, A, B).  Centroid offsets 0, 4.75, 5.25, 10.25
    over an extent of 10.25 quantise to 0, 474, 524, 1023: the top x bit (512) parts them in the middle, LBVH = ((A, B), (C, D)).
    PLOC: B u C is 1.5 wide and the least union of both, so they merge first; then A u BC = 6.25 against BC u D = 6.5:
    ((A, (B, C)), D).  The order is (A, B, C, D) = (2, 3, 0, 1) for both."""
    v = _row([(5.25, 6.25), (10.25, 11.25), (0, 1), (4.75, 5.75)])
    order, nodes = R.build("lbvh", v, 1)
    assert order.tolist() == [2, 3, 0, 1] and _nested(order, nodes) == (((2,), (3,)), ((0,), (1,)))
    order, nodes = R.build("ploc", v, 1)
    assert order.tolist() == [2, 3, 0, 1] and _nested(order, nodes) == (((2,), ((3,), (0,))), (1,))
    assert R.binary("ploc", v).rounds == [4, 3, 2]
    assert _nested(*R.build("lbvh", v, 3)) == ((2, 3), (0, 1)) and _nested(*R.build("ploc", v, 3)) == ((2, 3, 0), (1,))
    order, nodes = R.build("ploc", v, 3)
    l, r = int(nodes[1, 0]), int(nodes[1, 1])
    assert nodes[l, :4].tolist() == [0, 0, 3, 0] and nodes[r, :4].tolist() == [0, 0, 1, 3]
    assert _box(nodes, l) == [0, 0, 0, 6.25, 1, 0] and _box(nodes, r) == [10.25, 0, 0, 11.25, 1, 0]


def test_four_equal_triangles_in_a_row_by_hand():
    """The tie rule: unit triangles at x = 0, 1, 2, 3.  All neighbours' unions are 2 wide.  The pairs at distance 1 start at
    positions 0, 1, 2, and (low / 1) & 1 prefers 0 and 2: (0, 1) and (2, 3) merge in ONE round, then the two halves."""
    v = _row([(0, 1), (1, 2), (2, 3), (3, 4)])
    t = R.binary("ploc", v)
    assert t.rounds == [4, 2] and _nested(*t.emit(1)) == (((0,), (1,)), ((2,), (3,)))
    # seven in a row: (0,1) (2,3) (4,5) merge, 6 waits (its only tie-free choice, 5, is taken)
    t = R.binary("ploc", _row([(k, k + 1) for k in range(7)]))
    assert t.rounds[:2] == [7, 4]
