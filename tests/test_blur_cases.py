"""What tests/blur_cases.py covers (no GPU): every blur radius 1..31, the small
row formula in k_blur and in the pyramid tail, every tail radius class, the
layer counts the rest of the suite leaves out, and enough keypoints for the
sweep's keypoint comparison to mean something.  The radii are the oracle's
(blur_cases.radii), so this also pins the table against a change of the taps
rule; the library only has to accept every row (host logic of sift_hip_create).
"""
import pytest

import blur_cases as bc

ALL = {c: bc.radii(c) for c in bc.CASES}


def test_every_radius_is_a_layer_blur():
    seen = set()
    for init, layers in ALL.values():
        seen.update(layers)
        assert 1 <= init <= bc.MAX_RADIUS and 1 <= min(layers) and max(layers) <= bc.MAX_RADIUS, (init, layers)
    assert seen == set(range(1, bc.MAX_RADIUS + 1)), sorted(set(range(1, bc.MAX_RADIUS + 1)) - seen)


def test_case_table_is_small_and_distinct():
    assert len(set(bc.CASES)) == len(bc.CASES) <= 14


@pytest.mark.parametrize("r", [1, 2])
def test_small_row_formula_runs_in_the_tail(r):
    """2R + 1 <= 5 takes another row formula, in k_blur and in the tail: a
    configuration the tail takes (<= 6 layers, radii <= 16) has the radius."""
    assert any(r in layers and c[1] <= 6 and bc.tail_class(layers) is not None for c, (_, layers) in ALL.items())


def test_small_row_formula_runs_in_k_blur_without_tail():
    assert any(1 in layers and 2 in layers and bc.tail_class(layers) is None for _, layers in ALL.values())


def test_radius_one_initial_blur():
    assert any(init == 1 for init, _ in ALL.values())
    assert any(init == 1 and c[2] for c, (init, _) in ALL.items()), "the doubled base's sig_diff floor (0.1)"


def test_layer_counts():
    assert {1, 2, 4, 5} <= {c[1] for c in bc.CASES}  # 3, 6, 7, 9: the rest of the suite


@pytest.mark.parametrize("rp", bc.TAIL_CLASSES)
def test_every_tail_class(rp):
    assert any(bc.tail_class(layers) == rp for _, layers in ALL.values())


def test_large_radii_on_small_octaves():
    """Radii > 16 keep the tail off, so k_blur gets the 12- and 6-pixel octaves: planes narrower than R."""
    assert any(max(layers) > bc.TAIL_RMAX for _, layers in ALL.values())
    assert min(bc.SWEEP_W, bc.SWEEP_H) >> 5 < bc.TAIL_RMAX


def test_one_bounce_cases():
    """A configuration per LDS layout class (max radius <= 8, 9..24, > 24), none of them taken by the
    tail, with frame sizes on both sides of W > R + 1 && H > R + 1 and no side below 2."""
    mx = []
    for c in bc.ONE_BOUNCE_CASES:
        init, layers = ALL[c]
        assert bc.tail_class(layers) is None, c
        mx.append(max(layers + [init]))
        sizes = bc.one_bounce_sizes(c)
        assert len(sizes) == 8 and min(min(wh) for wh in sizes) >= 2
        for r in (min(layers + [init]), max(layers + [init])):
            assert any(w > r + 1 and h > r + 1 for w, h in sizes) and any(w <= r + 1 for w, h in sizes) \
                and any(h <= r + 1 for w, h in sizes)
    assert mx[0] <= 8 and 9 <= mx[1] <= 24 and mx[2] > 24, mx


def test_four_wave_and_negative_cases():
    layers = set(ALL[bc.FOUR_WAVE_CASE][1])
    assert len(layers - {5, 6, 8, 10, 13}) >= 4 and max(layers) <= 24  # radii the default pyramid never runs
    assert bc.tail_class(ALL[bc.NEGATIVE_CASE][1]) == 16


def test_library_accepts_every_case(sift):
    for c in bc.CASES:
        det = sift.Detector(sift.CudaSiftConfig(col_width=bc.SWEEP_W, row_width=bc.SWEEP_H, **bc.config_kwargs(c)), device=0)
        assert det.nOctaves == bc.oracle.num_octaves(bc.SWEEP_W, bc.SWEEP_H, bc.oracle_params(c)) >= 6, c


def test_oracle_runs_every_case(sift):
    counts = {bc.case_id(c): len(bc.oracle_keypoints(sift, c)[0]) for c in bc.CASES}
    print(counts)
    assert sum(n > 20 for n in counts.values()) * 2 >= len(counts), counts
