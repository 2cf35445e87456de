"""Oracle-only controls of tests/test_single_light_gpu.py (no GPU): that its scenes and its statistic can fail.
 - the scenes of one delta light listed n times: direct lighting is a non-zero share of the pixels compared, and one light fewer moves the oracle's film by more
   than 20 x the tolerance the GPU test allows (tests/test_scene_limits.py's test_every_sentinel_decides_the_picture is the model);
 - the z statistic at STAT_SPP samples: the oracle's both_mis against itself under another seed passes with room, and the oracle with the pick probability left
   out (its film with the direct part n-fold) fails."""
import numpy as np
import pytest

from single_light_scenes import STAT_SPP, luminance, repeated_delta_scene, stat_case, z_scores, z_verdict

DEBUG_TOL = 1e-4     # tests/test_parity_gpu.py's debug-sampler frames: pixels may differ by 1e-4


@pytest.mark.parametrize("kind", ["point", "direction"])
def test_repeated_delta_scenes_are_not_trivial(kind, A, api, O):
    W, H = 48, 40
    scene = repeated_delta_scene(A, api, O, kind, W, H)
    n = scene.scene.light_count
    assert n == (3 if kind == "point" else 4)
    both = O.render(scene, api.make_params(W, H, 2, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_BOTH_MIS))
    idle = O.render(scene, api.make_params(W, H, 2, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_IDLE))
    direct = np.abs(both - idle).max(axis=2)
    assert float((both >= 1.0).mean()) < 0.02                 # next to nothing clamped: a light more or less shows wherever it reaches
    share = float((direct > 20 * DEBUG_TOL).mean())
    print("%s x %d: direct lighting beyond 20 x tolerance on %.0f %% of the pixels, film mean %.3f" % (kind, n, 100 * share, both.mean()))
    assert share > 0.25 and idle.max() == 0.0                 # (delta lights only: without direct lighting nothing is lit at all)
    scene.scene.light_count = n - 1                           # one of the repeated lights dropped: what a wrong pick count or a wrong factor n amounts to
    fewer = O.render(scene, api.make_params(W, H, 2, sampler=A.SAMPLER_DEBUG, direct_sample=A.DIRECT_BOTH_MIS))
    scene.scene.light_count = n
    moved = np.abs(fewer - both).max(axis=2)
    print("  one light fewer: %.0f %% of the pixels move by more than 20 x tolerance, largest %.3f" % (100 * float((moved > 20 * DEBUG_TOL).mean()), moved.max()))
    assert float((moved > 20 * DEBUG_TOL).mean()) > 0.25      # a quarter of the film, against the 0.2 % of pixels the GPU test lets differ by 1e-4


def _oracle_luminances(O, scene, p, pixels):
    return np.stack([luminance(O.li(scene, p, x, y, 0, p.samples_per_pixel)) for (x, y) in pixels])


@pytest.mark.parametrize("which", ["veach", "cornell_lamp_point"])
def test_statistic_passes_the_control_and_fails_the_counter_example(which, A, api, O):
    """Measured at STAT_SPP = 1024 (|mean z| in standard errors of the mean, share of pixels beyond |z| = 4; the bounds are 4 and 1 %):
         Veach (280 of 288 pixels vary)              control 0.40, 0 %      n x direct 376, 98 %
         Cornell lamp + point (334 of 336 vary)      control 1.26, 0 %      n x direct 225, 94 %"""
    scene, W, H, pixels = stat_case(which, A, api)
    n = scene.c.light_count
    assert len(pixels) >= 256 and n > 1
    a = _oracle_luminances(O, scene, api.make_params(W, H, STAT_SPP, seed=1234), pixels)
    b = _oracle_luminances(O, scene, api.make_params(W, H, STAT_SPP, seed=4321), pixels)
    z, fixed = z_scores(a, b)
    ok, mean_in_se, share = z_verdict(z)
    print("%s control: %d pixels vary, |mean z| = %.2f standard errors, %.2f %% beyond 4, fixed pixels differ by %.1e" % (which, len(z), mean_in_se, 100 * share, fixed))
    assert len(z) >= 256 and fixed <= 1e-4
    assert ok and mean_in_se < 2.0 and share == 0.0, (mean_in_se, share)           # "with room": half the bound, no pixel in the tail
    # the pick probability left out: every sample's direct part n-fold (the path does not depend on the strategy, so idle under the same seed is its indirect part)
    idle = _oracle_luminances(O, scene, api.make_params(W, H, STAT_SPP, seed=1234, direct_sample=A.DIRECT_IDLE), pixels)
    wrong = idle + n * (a - idle)
    zw, _ = z_scores(wrong, b)
    ok, mean_in_se, share = z_verdict(zw)
    print("%s n x direct: |mean z| = %.2f standard errors, %.2f %% beyond 4" % (which, mean_in_se, 100 * share))
    assert not ok and mean_in_se > 10 * 4.0 and share > 10 * 0.01, (mean_in_se, share)
