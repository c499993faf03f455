"""The bars of tests/gpu_checks.py, pinned from the outside on synthetic films and counters: no device is needed to see that check_bar,
check_counts and differing_share accept and refuse what DESIGN.md 9.2 says they do."""
import numpy as np
import pytest

from gpu_checks import check_bar, check_counts, differing_share

N = 1000                         # the films are 8 x 8, except where a share is asked for: 0.4 % and 1 % are whole pixels of 40 x 25


def film(h=8, w=8):
    rng = np.random.default_rng(1)
    return rng.random((h, w, 3)).astype(np.float32), np.ones((h, w), np.float32)


def refused(*args):
    with pytest.raises(AssertionError):
        check_bar("synthetic", *args)


def test_check_bar_passes_an_identical_film_under_both_bars():
    rgb, alpha = film()
    for loose in (False, True):
        m = check_bar("same", rgb.copy(), alpha.copy(), rgb, alpha, loose)
        assert m["maxabs"] == 0.0 and m["frac"] == 1.0 and m["alpha_maxabs"] == 0.0 and m["alpha_off"] == 0.0


def test_check_bar_strict_refuses_one_pixel_off_by_2e_5():
    rgb, alpha = film()
    rgb[:] = np.float32(0.5)                    # 2e-5 is 671 float32 steps at .5: the offset survives the rounding
    off = rgb.copy(); off[3, 4, 1] += np.float32(2e-5)
    refused(off, alpha, rgb, alpha, False)
    check_bar("colour, loose", off, alpha, rgb, alpha, True)
    aoff = alpha.copy(); aoff[5, 2] -= np.float32(2e-5)
    refused(rgb, aoff, rgb, alpha, False)
    refused(rgb, aoff, rgb, alpha, True)                            # one pixel of 64 is 1.6 % of them: more than the loose bar's 0.5 %


def test_check_bar_loose_takes_4_per_mille_of_the_pixels_off_and_refuses_1_per_cent():
    rgb, alpha = film(40, 25)
    flat = lambda a: a.reshape(N, -1)
    for n_off, passes in ((4, True), (10, False)):
        off = rgb.copy(); flat(off)[:n_off, 0] += np.float32(1e-2)
        aoff = alpha.copy(); flat(aoff)[:n_off, 0] -= np.float32(1e-2)
        if passes:
            m = check_bar("colour", off, alpha, rgb, alpha, True)
            assert m["frac"] == (N - n_off) / N
            assert check_bar("alpha", rgb, aoff, rgb, alpha, True)["alpha_off"] == n_off / N
        else:
            refused(off, alpha, rgb, alpha, True)
            refused(rgb, aoff, rgb, alpha, True)
        refused(off, alpha, rgb, alpha, False)
        refused(rgb, aoff, rgb, alpha, False)


def test_check_bar_loose_refuses_a_mean_l2_of_1e_4():
    """few pixels off, but far: the mean clause"""
    rgb, alpha = film(40, 25)
    off = rgb.copy(); off[0, 0, 0] += np.float32(0.2)               # one pixel of 1000: frac .999, mean L2 2e-4
    refused(off, alpha, rgb, alpha, True)


def test_check_bar_refuses_a_nan_in_alpha_or_colour():
    rgb, alpha = film()
    bad = alpha.copy(); bad[2, 2] = np.nan
    badrgb = rgb.copy(); badrgb[2, 2, 0] = np.inf
    for loose in (False, True):
        refused(rgb, bad, rgb, alpha, loose)
        refused(badrgb, alpha, rgb, alpha, loose)


def stats(closest=100_000, any_=30_000, cam="4225"):
    return dict(closest_rays=closest, any_rays=any_, stats={"Camera Rays Traced": cam})


def counters(closest=100_000, any_=30_000, cam=4225, bad=0):
    return dict(camera_rays=cam, closest_rays=closest, any_rays=any_, bad_samples=bad)


def counts_refused(cnt, st, loose):
    with pytest.raises(AssertionError):
        check_counts("synthetic", cnt, st, loose)


def test_check_counts_strict_refuses_a_difference_of_one():
    check_counts("equal", counters(), stats(), False)
    for d in (-1, 1):
        counts_refused(counters(closest=100_000 + d), stats(), False)
        counts_refused(counters(any_=30_000 + d), stats(), False)


def test_check_counts_loose_tolerance_is_each_counter_s_own():
    """max(4, int(2e-4 * n)): 20 for 100 000 closest-hit rays, 6 for 30 000 shadow rays, 4 below 25 000"""
    for d in (-1, 1):
        check_counts("closest at tol", counters(closest=100_000 + 20 * d), stats(), True)
        counts_refused(counters(closest=100_000 + 21 * d), stats(), True)
        check_counts("any at tol", counters(any_=30_000 + 6 * d), stats(), True)
        counts_refused(counters(any_=30_000 + 7 * d), stats(), True)            # inside the closest-hit count's 20: not this counter's bound
        check_counts("floor", counters(closest=1000 + 4 * d, any_=0), stats(closest=1000, any_=0), True)
        counts_refused(counters(closest=1000 + 5 * d, any_=0), stats(closest=1000, any_=0), True)
        counts_refused(counters(closest=1000, any_=5), stats(closest=1000, any_=0), True)


def test_check_counts_refuses_a_bad_sample():
    for loose in (False, True):
        counts_refused(counters(bad=1), stats(), loose)


def test_check_counts_takes_camera_rays_as_statsprint_wrote_them():
    """exact where the string is ("17424"); where StatsPrint abbreviated ("17.4k"), equal as printed: stat_int's .0005 * n + 50"""
    for loose in (False, True):
        check_counts("exact", counters(cam=17424), stats(cam="17424"), loose)
        counts_refused(counters(cam=17425), stats(cam="17424"), loose)
        check_counts("abbreviated", counters(cam=17424), stats(cam="17.4k"), loose)
        check_counts("abbreviated, at the bound", counters(cam=17400 + 58), stats(cam="17.4k"), loose)       # .0005 * 17400 + 50 = 58.7
        counts_refused(counters(cam=17400 + 59), stats(cam="17.4k"), loose)
        counts_refused(counters(cam=17400 - 59), stats(cam="17.4k"), loose)
        check_counts("millions", counters(cam=1_050_000), stats(cam="1.05M"), loose)
        counts_refused(counters(cam=1_052_000), stats(cam="1.05M"), loose)


def test_differing_share_counts_the_pixels_more_than_1e_3_away():
    rgb, _ = film()
    assert differing_share(rgb, rgb) == 0.0
    off = rgb.copy()
    off[:2] += np.float32(2e-3)                 # 16 of 64 pixels, L2 = 2e-3 * sqrt(3)
    off[2, 0, 0] += np.float32(5e-4)            # and one below the threshold
    assert differing_share(off, rgb) == 0.25
