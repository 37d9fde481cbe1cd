"""What the float64 arm of smooth shading (tests/smooth_spec.py) reaches by itself on the cases tests/test_gpu_smooth.py compares on the
device (tests/smooth_cases.py): every `need` table is half the arm's own count, tag by tag, every smooth tag the case is meant to reach
is in its table, and the samples left out stay under the caps - bssrdf-coplanar at most 5 %, smooth-undecided at most 2 %: conditions on
the scenes and the camera, checked inside smooth_cases.run.  No GPU: compare_arm counts with count_only=True."""
import numpy as np
import pytest

import smooth_cases as SC
import smooth_spec as spec

MEANT = {"jade": ("smooth", "smooth-flat", "smooth-side", "smooth-redirect", "smooth-culled"), "glass": ("smooth", "smooth-redirect"),
         "diffuse": ("smooth", "smooth-culled"), "jade_sky_importance": ("smooth", "smooth-side", "smooth-culled"),
         "jade_cosine": ("smooth", "smooth-culled"), "bent_patchwork": ("smooth", "smooth-side", "smooth-redirect", "smooth-culled")}


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_the_need_table_is_half_of_what_the_arm_counts(name):
    seen, bad, n, skipped, left = SC.run(name)
    need = SC.CASES[name]["need"]
    assert bad == 0 and n + skipped == SC.SIZE * SC.SIZE * len(SC.FRAMES)
    assert skipped == left["coplanar"] + left["undecided"]
    print(name, left, dict(sorted(seen.items())))
    for tag in MEANT[name]:
        assert need.get(tag, 0) >= 1, f"{name}: '{tag}' is meant to be reached on the device"
    assert need == {t: c // 2 for t, c in seen.items() if c // 2 >= 1 and t in need}, (need, seen)
    assert set(need) >= {t for t, c in seen.items() if c >= 4}, "every tag the arm reaches four times or more is asked of the device"


def test_the_special_rows_take_the_rule_they_are_written_for():
    out = spec.normal_rows(spec.special_rows())
    R = spec
    assert list(out["rule"]) == [R.RULE_DEGENERATE, R.RULE_DEGENERATE, R.RULE_SUM, R.RULE_SUM, R.RULE_SUM, R.RULE_SUM, R.RULE_FLAT, R.RULE_FLAT,
                                 R.RULE_SIDE, R.RULE_SIDE, R.RULE_NS, R.RULE_NS, R.RULE_SIDE]
    g = spec.special_rows()[:, 18:21].astype(np.float64)
    fell = out["rule"] != R.RULE_NS
    assert np.array_equal(out["n"][fell], g[fell]), "a vertex that falls back takes g unchanged"


def test_the_random_rows_reach_every_rule_and_interpolate_exactly_at_the_corners():
    rows = spec.random_rows(4096)
    out = spec.normal_rows(rows)
    assert (out["rule"] == spec.RULE_NS).sum() > 2500 and (out["rule"] == spec.RULE_SIDE).sum() > 300
    assert out["clear"].mean() > 0.95 and out["D"][out["rule"] == spec.RULE_NS].max() < 1e-4
    at = rows.copy()
    at[:, 21:24] = at[:, 3:6]                          # p = p2: ns = n2 / |n2|
    at[:, 24:27] = at[:, 12:15] + at[:, 18:21] * 4     # r with both normals
    o2 = spec.normal_rows(at)
    n2 = at[:, 12:15].astype(np.float64)
    n2 /= np.sqrt((n2 * n2).sum(-1))[:, None]
    ok = o2["rule"] == spec.RULE_NS
    assert ok.sum() > 3000 and np.abs(o2["n"][ok] - n2[ok]).max() < 1e-9
