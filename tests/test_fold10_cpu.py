"""Planner rows of the folded F(4x4,3x3) tile of the 12x8 level, which holds ten slices per work item (csrc/rcu_plan.hip pick_config, csrc/rcu_wino4.hip):
through rcu_unet_plan, no GPU."""
import pytest

from plan_rows import plan_rows

FOLDED = 'conv3x3_winograd4<S8T12x8,N32,K8>'
STRIP = 'conv3x3_winograd<S8T4x8,N64,K8>'


# The 192x128 BraTS shape.  Plans of the pass-group launches (480 samples and up) count the folded kernel's rounds in groups of ten slices; smaller
# plans keep the decisions they had while a work item was eight slices -- rounds_4 * 1.35 < rounds_2 with both counted in groups of eight: 448 samples
# 4 against 6 rounds (taken), 400 samples 4 against 5, 320 samples 3 against 4, 160 samples 2 against 2, 8 samples 1 against 1 (not taken) -- because a
# 160-sample plan gives the bits of an 8-sample one (tests/test_gpu_fullsize.py).
@pytest.mark.parametrize('n,kernel', [(640, FOLDED), (480, FOLDED), (448, FOLDED), (400, STRIP), (320, STRIP), (160, STRIP), (8, STRIP)])
def test_bottom_level_kernel_by_plan_size(n, kernel):
    rows = plan_rows(192, 128, n)
    assert (rows[9]['height'], rows[9]['width']) == (12, 8) and rows[9]['name'].startswith('bottom_convs')
    assert [r['kernel'] for r in rows if (r['height'], r['width']) == (12, 8)] == [kernel, kernel]
    forced = plan_rows(192, 128, n, dict(conv_winograd4=2))
    assert [r['kernel'] for r in forced if (r['height'], r['width']) == (12, 8)] == [FOLDED, FOLDED]
    # nothing else of the plan depends on the rule
    assert [r['kernel'] for r in forced if (r['height'], r['width']) != (12, 8)] == [r['kernel'] for r in rows if (r['height'], r['width']) != (12, 8)]


def test_folded_kernel_reports_64_slots_per_60_tiles():
    for n in (640, 8):
        rows = [r for r in plan_rows(192, 128, n, dict(conv_winograd4=2)) if r['kernel'] == FOLDED]
        assert [(r['cin'], r['cout']) for r in rows] == [(256, 512), (512, 512)]
        for r in rows:
            six_tiles = 2.0 * r['cin'] * r['cout'] * 36.0 * 6.0          # 36 products per 4x4 tile, six tiles per 12x8 slice
            assert six_tiles == r['flops'] / 4.0                          # F(4x4,3x3): 36 / 16 of the direct form's 9 multiplications per pixel
            assert r['mfma_flops'] == pytest.approx(six_tiles * 64.0 / 60.0, rel=1e-12)
