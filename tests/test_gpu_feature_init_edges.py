"""The feature-initialisation image operators at every tile, cap and tie edge (feature_init_cases.py): the Shi-Tomasi
detector (k_find_best_patch) and the multi-ellipse search in all its forms (k_me_search, k_me_big_scores, k_me_big_argmin)
against the oracle, bit for bit - integer positions, FP64 eigenvalues and scores compared with ==.  Every test first asserts
the condition that proves its case reaches the edge it names."""
import numpy as np
import pytest

import feature_init_cases as fic
import oracle_api as oa

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", fic.DETECTOR_CASE_NAMES)
def test_detector_edge(name):
    from scenelib2_amd import improc
    case = fic.detector_case(name)
    want = case.oracle(oa)
    case.check(want)
    uv, ev = improc.find_best_patch_batch(case.images, case.idx, case.regions, case.uv_in)
    for t, (wu, wv, wev) in enumerate(want):
        assert (uv[t, 0], uv[t, 1]) == (wu, wv) and ev[t] == wev, (name, t, list(case.regions[t]), int(case.idx[t]), uv[t], ev[t], want[t])


@pytest.mark.parametrize("name", fic.MULTI_ELLIPSE_CASE_NAMES)
def test_multi_ellipse_edge(name):
    from scenelib2_amd import improc
    case = fic.multi_ellipse_case(name, oa)
    want = case.oracle(oa)
    case.check(want)
    res, corr = improc.search_multiple_overlapping_ellipses_batch(case.images, case.idx, case.patches, case.counts, case.pu, case.ce)
    for j, (wres, wcorr, _) in enumerate(want):
        sl = case.sl(j)
        bad = (res[sl] != wres).any(axis=1) | (corr[sl] != wcorr)
        assert not bad.any(), (name, j, case.form(j), np.nonzero(bad)[0][:8], res[sl][bad][:8], wres[bad][:8], corr[sl][bad][:8], wcorr[bad][:8])


def test_multi_ellipse_edges_in_one_call_and_again():
    """All cases that share the 96 x 72 frame as ONE batch (every form side by side in a launch, the many-workgroup list
    longer than its grid), twice: the second call must not see anything of the first."""
    from scenelib2_amd import improc
    cases = [fic.multi_ellipse_case(n, oa) for n in ("counts", "area", "novalid", "bigjobs", "borders big", "truncation", "lowsigma")]
    images = np.concatenate([c.images for c in cases])
    base = np.cumsum([0] + [len(c.images) for c in cases])
    idx = np.concatenate([c.idx + base[k] for k, c in enumerate(cases)])
    patches, counts = np.concatenate([c.patches for c in cases]), np.concatenate([c.counts for c in cases])
    pu, ce = np.concatenate([c.pu for c in cases]), np.concatenate([c.ce for c in cases])
    wres = np.concatenate([w[0] for c in cases for w in c.oracle(oa)])
    wcorr = np.concatenate([w[1] for c in cases for w in c.oracle(oa)])
    assert sum(c.form(j) == "big" for c in cases for j in range(len(c.counts))) > 2 * fic.ME_BIG_GRID_Y
    for _ in range(2):
        res, corr = improc.search_multiple_overlapping_ellipses_batch(images, idx, patches, counts, pu, ce)
        assert (res == wres).all() and (corr == wcorr).all(), np.nonzero((res != wres).any(axis=1) | (corr != wcorr))[0][:16]
