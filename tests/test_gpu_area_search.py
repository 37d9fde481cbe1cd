"""The BSSRDF branch's exit-triangle search on the device, alone and exact.

exit_search (jade_shade.h) replaces the reference's bisection of the prefix areas (PathTrace.cu:1031-1048) by a table cell, a short
scan and a replay of the bisection on indices; bounce_branch calls it with one draw.  libjade_hip_debug.so's jade_debug_exit_search
runs it one thread per row, and every row must give the reference's LAST midpoint (tests/area_search_ref.py: ref_search, the oracle's
loop in float32 numpy) and index_mapping of it - no tolerance, nothing left out.  Frames only meet this search at random u; the rows
here are the events of probability 2^-24 a frame never draws: u = 0 and 1.0f, every cell boundary of the table and the floats
around it, fl(u A) exactly on a prefix area, zero-area runs, and the objects without a table, which bisect on the device."""
import numpy as np
import pytest

import area_search_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    obj, u = A.all_rows()
    return obj, u, A.reference_rows(obj, u)


@pytest.fixture(scope="module", params=A.MAPPINGS)
def searched(request, hip_debug, rows):
    obj, u, _ = rows
    hs = A.search_scene(request.param)
    with hip_debug.scene(hs) as sc:
        middle, mapped = A.search_device(sc, obj, u)
    return hs, middle, mapped


def test_every_row_is_the_reference_midpoint(searched, rows):
    obj, u, want = rows
    hs, middle, mapped = searched
    bad = np.flatnonzero(middle != want)
    per_object = {A.PREFIX_SETS[o][0]: int((obj[bad] == o).sum()) for o in np.unique(obj[bad])}
    print(f"{len(u)} rows over {len(A.PREFIX_SETS)} objects: {len(bad)} differ {per_object}")
    assert len(bad) == 0, [(A.PREFIX_SETS[obj[i]][0], float(u[i]), int(middle[i]), int(want[i])) for i in bad[:8]]
    assert np.array_equal(mapped, hs.a["mapping"][want]), "out_mapped is index_mapping[middle]"


def test_the_mapping_is_applied_and_not_the_midpoint_returned(searched, rows):
    hs, middle, mapped = searched
    m = hs.a["mapping"]
    if (m == np.arange(len(m))).all():
        assert np.array_equal(mapped, middle)
    elif (m == m[0]).all():
        assert (mapped == m[0]).all() and (middle != m[0]).any()
    else:
        assert (mapped != middle).mean() > 0.9


def test_the_rows_reach_what_they_are_meant_to_reach(rows):
    """Every object is searched, the table objects at both ends of [0, 1]; the objects of one and two triangles come back as 0 and the
    others stay inside their segment, strictly between its ends (a midpoint of left < right - 1 is neither)."""
    obj, u, want = rows
    segs = A.segments()
    for o, ((name, p), (b, e)) in enumerate(zip(A.PREFIX_SETS, segs)):
        m = obj == o
        assert m.sum() >= 6000 and u[m].min() == 0 and u[m].max() == 1, name
        if len(p) < 3:
            assert (want[m] == 0).all(), name
        else:
            assert (want[m] > b).all() and (want[m] < e).all(), name
            if name not in ("nan_inside", "inf_last", "all_zero", "over_the_bar", "descending"):  # (these end at one midpoint whatever u is)
                assert len(np.unique(want[m])) >= min(len(p) - 2, 2), name


def test_the_entry_point_refuses_rows_outside_the_table_before_any_launch(hip_debug):
    from jaderaytracerendering_amd import _abi
    fn = A.exit_search_fn(hip_debug.lib)
    out = np.zeros(2, np.int32)
    with hip_debug.scene(A.search_scene()) as sc:
        n_obj = len(A.PREFIX_SETS)
        for obj, u in (([0, n_obj], [0.5, 0.5]), ([0, -1], [0.5, 0.5]), ([0, 1], [0.5, np.nextafter(np.float32(1), np.float32(2))]),
                       ([0, 1], [np.nan, 0.5]), ([0, 1], [-1e-30, 0.5])):
            o, v = np.int32(obj), np.float32(u)
            assert fn(sc._h, 2, o.ctypes.data, v.ctypes.data, out.ctypes.data, out.ctypes.data) == _abi.JADE_ERR_INVALID, (obj, u)
        middle, mapped = A.search_device(sc, np.int32([1, 1]), np.float32([0, 1]))
        b = int(A.segments()[1, 0])
        assert middle.tolist() == [b + 1, b + 1] and mapped.tolist() == [b + 1, b + 1]  # t3: one midpoint
