"""prepare_scene on caller-shaped trees, without a GPU ("caller-shaped trees").

jade_scene_create walks the caller's node array from node 1 (validate_desc) and then lays it out for the kernels (prepare_scene,
jade_scene_prep.hip: host code, no HIP call).  libjade_hip_debug.so's jade_debug_prepare_scene_host runs exactly those two on a
descriptor and returns the records; here every shape of tests/tree_shapes.py is held against tests/prep_ref.py's statement of what
the records must be, and a float32 walk of the PREPARED records is held against the oracle ray by ray - so that nothing reaches a
device (tests/test_gpu_tree_shapes.py imports the same list) whose references have not been shown to stay inside the arrays."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import B, ROOT
from jaderaytracerendering_amd import _abi

import prep_ref as P
import tree_shapes as TS
import walk_ref as W


@pytest.fixture(scope="module")
def dbg():
    path = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
    assert os.path.exists(path), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    return C.CDLL(path)


_prepared = {}


def _prep(dbg, name, wide):
    if (name, wide) not in _prepared:
        hs = TS.base_scene(name) if name in TS.BASES else TS.scene(name)
        rc, p = P.prepare(dbg, hs, wide)
        assert rc == 0, (name, rc)
        _prepared[name, wide] = p
    return _prepared[name, wide]


def _two_triangle_tree(hs, tail):
    """root -> two leaves of one triangle, and `tail` behind them."""
    nodes = W.tree_nodes(W.node(W.leaf(0), W.leaf(1)), hs.vertices())
    return TS._with_nodes(hs, np.concatenate([nodes, tail]), 2)


def test_unused_nodes_behind_a_two_triangle_tree_are_not_read(dbg):
    """A node array with spare capacity behind the tree.  Before the root's reach was computed, prepare_scene looped over every node:
    two zero-filled spare nodes gave n_internal = 3 and missing_child (the general walk, no wide records, no occluder cache), a spare
    "leaf" at triangle 400 000 000 and a spare node with children 400 000 000 / -7 were read out of bounds."""
    hs = TS.base_scene("base")
    want = P.prepare(dbg, _two_triangle_tree(hs, np.zeros((0, 10), np.uint32)))[1]
    assert (want.n_internal, want.n_pairs, want.missing_child, want.nested) == (1, 2, 0, 1) and len(want.nodes4) == 1
    far_leaf = np.zeros((1, 10), np.uint32)
    far_leaf.view(np.int32)[0, 2:4] = 3, 400000000
    far_kids = np.zeros((1, 10), np.uint32)
    far_kids.view(np.int32)[0, :2] = 400000000, -7
    for tail in (np.zeros((2, 10), np.uint32), far_leaf, far_kids):
        rc, got = P.prepare(dbg, _two_triangle_tree(hs, tail))
        assert rc == 0 and got.raw() == want.raw()


def test_a_node_named_by_both_child_slots_gets_one_record(dbg):
    """root -> x, x with x = an internal node over two leaves: two distinct internal nodes, two records (there were three, the first an
    all-zero record whose references decode as "internal node 0"); root -> the same leaf twice: the other leaf, unused, is not counted."""
    hs = TS.base_scene("base")
    x = W.node(W.leaf(0), W.leaf(1))
    rc, p = P.prepare(dbg, W.with_tree(hs, W.node(x, x)))
    assert rc == 0 and p.n_internal == 2 and p.n_pairs == 2
    assert int(p.nodes[0, 3, 0]) == int(p.nodes[0, 3, 1]) == 1 and p.nodes[1].any()
    P.check_records(W.with_tree(hs, W.node(x, x)), p, 1)
    two = _two_triangle_tree(hs, np.zeros((0, 10), np.uint32))
    two.a["nodes"].view(np.int32)[1, 1] = two.a["nodes"].view(np.int32)[1, 0]
    rc, p = P.prepare(dbg, two)
    assert rc == 0 and p.n_internal == 1 and p.n_pairs == 1
    P.check_records(two, p, 1)


@pytest.mark.parametrize("name", TS.BASES + TS.ACCEPTED)
def test_records_are_the_statement(dbg, name):
    """Refs and counts, child boxes and pair records, the order of the internal records, the wide records and the flags
    (prep_ref.check_records), with and without wide records."""
    hs = TS.base_scene(name) if name in TS.BASES else TS.scene(name)
    for wide in (0, 1):
        P.check_records(hs, _prep(dbg, name, wide), wide)
    assert len(_prep(dbg, name, 0).nodes4) == 0
    if name in TS.BASES:
        assert len(_prep(dbg, name, 1).nodes4) == _prep(dbg, name, 1).n_internal > 0  # (the bases themselves are nested and complete)


@pytest.mark.parametrize("name", [s.name for s in TS.SHAPES if s.same_as_base])
def test_unused_nodes_and_node_numbers_change_nothing(dbg, name):
    """tail, renumbered (and n = -5 for n = 0): the prepared arrays and every derived fact are the base tree's, byte for byte."""
    base = TS.BY_NAME[name].base
    for wide in (0, 1):
        got, want = _prep(dbg, name, wide), _prep(dbg, base, wide)
        assert got.raw() == want.raw()


@pytest.mark.parametrize("name", TS.REFUSED)
def test_one_visit_past_the_budget_is_refused_by_both_backends(dbg, oracle, name):
    """(The HIP module validates before it looks for a device, so its answer is the same with and without one.)"""
    sh, hs = TS.BY_NAME[name], TS.scene(name)
    assert P.prepare(dbg, hs)[0] == sh.refused == _abi.JADE_ERR_UNSUPPORTED
    for be in (oracle, B.Backend(os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip.so"))):
        with pytest.raises(B.JadeError) as ei:
            be.scene(hs)
        assert ei.value.code == sh.refused
    exact = TS.scene("budget-exact")
    assert TS.walk_visits(exact.a["nodes"])[0] == 4 * exact.n_nodes + 8
    with oracle.scene(exact):
        pass


_tables = {}


def _table(oracle, name):
    """prep_ref.triangle_table for the shape's rays; shapes of one base with the same rays share it."""
    hs, (o, d, _) = TS.scene(name), TS.rays(name)
    key = (TS.BY_NAME[name].base, o.tobytes(), d.tobytes())
    if key not in _tables:
        _tables[key] = P.triangle_table(oracle, hs, o, d)
    return _tables[key]


@pytest.mark.parametrize("name", TS.ACCEPTED)
def test_a_walk_of_the_prepared_records_is_the_oracles(dbg, oracle, name):
    """4096 rays per shape (tree_shapes.rays): walk_ref's rules applied to the records prepare_scene made - its references, its child boxes,
    the triangle numbers of its pair records - give the oracle's triangle, the bits of its distance, and its counts of node records
    and triangle tests, ray by ray.  The oracle alone finds at least 100 hits and 100 misses in every set (a tree that covers nothing:
    misses only), never a triangle that no reachable leaf holds, and - where every box contains what lies under it - what a scan
    over the covered triangles finds.  Shapes that leave triangles out have 512 rays aimed at those."""
    sh, hs = TS.BY_NAME[name], TS.scene(name)
    o, d, skip = TS.rays(name)
    assert len(o) == TS.N_RAYS
    wi, wt, _, wv, wn = P.reference(oracle, name)
    hitm = wi >= 0
    cov = TS.covered(hs.a["nodes"], hs.n_triangles)
    if sh.empty:
        assert not cov.any() and not hitm.any()
    else:
        assert hitm.sum() >= 100 and (~hitm).sum() >= 100, (int(hitm.sum()), int((~hitm).sum()))
    assert cov[wi[hitm]].all(), "a triangle in no reachable leaf is never hit"
    if name.startswith("uncovered"):
        assert (~cov).sum() >= 10 and TS.AIMED_AT_UNCOVERED >= 100
        lost = set(np.flatnonzero(~cov).tolist())
        assert lost & set(hs.a["emit"].tolist()) and lost & set(hs.a["mapping"].tolist())
    hit, dist = _table(oracle, name)
    gi, gt, gv, gn = P.walk_records(_prep(dbg, name, 0), o, d, skip, hit, dist)
    assert np.array_equal(gi, wi), "triangle"
    assert np.array_equal(gt.view(np.uint32), wt.view(np.uint32)), "distance bits"
    assert np.array_equal(gv, wv), "node records per ray"
    assert np.array_equal(gn, wn), "triangle tests per ray"
    if sh.honest:
        # (a box is entered iff its slab value is > 0: a ray that leaves from a box's own face never enters it, whatever rounding makes
        # of the triangles in that face - so the scan is over the leaves whose OWN box the ray enters; nested boxes and a monotone
        # slab test, tests/test_box_monotone.py, then take the walk down to every one of them)
        ni, nf = hs.node_i32(), hs.node_f32()
        leaves = [i for i in TS.reachable(hs.a["nodes"])[0] if ni[i, 2] > 0]
        entered = np.zeros((hs.n_triangles, len(o)), bool)
        with np.errstate(invalid="ignore"):
            for k in range(len(o)):
                met = W.slab(nf[leaves, 4:7], nf[leaves, 7:10], o[k], d[k]) > 0
                for i in leaves if leaves == [1] else np.asarray(leaves)[met]:  # (a root that is a leaf: its box is never tested)
                    entered[ni[i, 3]:ni[i, 3] + ni[i, 2], k] = True
        cand = np.where(hit & entered, dist, P.INF)
        cand[skip[skip >= 0], np.flatnonzero(skip >= 0)] = P.INF
        flat = cand.min(0)
        assert np.array_equal(flat.view(np.uint32), wt.view(np.uint32)), "honest boxes: the walk finds what a scan of the leaves it can enter finds"
        alone = hitm & ((cand == flat[None, :]).sum(0) == 1)
        assert np.array_equal(cand.argmin(0)[alone], wi[alone])
