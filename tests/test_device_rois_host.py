"""CPU tests of ``evam_pp_ssd_rois_host``: the shared detection-row arithmetic (``ssd_row_rect``, csrc/evam_geom.h)
against the Python chain a detect -> classify pipeline runs on the host (tests/device_rois_cases.py). The rects and
their order must be equal: the device path lists what the host path lists, so a classifier row can be attached to
the j-th region the host builds."""
import zlib

import numpy as np
import pytest

import device_rois_cases as C


def seed_of(case):
    return zlib.crc32(repr(case).encode())


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_host_helper_equals_python_chain(evam, case):
    n, K, kind, labels = case
    seen = 0
    for rep in range(3):
        b = C.make_batch(evam, seed_of(case) + rep, n, K, kind, labels)
        want = C.python_rois(evam, b)
        got, count = C.host_rois(evam, b)
        assert count == len(want), f"{C.case_id(case)} rep {rep}: count {count}, Python lists {len(want)}"
        assert [tuple(r) for r in got.tolist()] == want, f"{C.case_id(case)} rep {rep}"
        seen += count
    if n * K >= 30:
        assert seen > 0, "the case accepts nothing: it checks nothing"


def test_cases_hold_the_edges(evam):
    """The generator produces what the issue lists: rows at the threshold, terminators with live rows behind them,
    empty items, rects starting on a .5 product, reversed and zero-area boxes, boxes outside [0, 1]."""
    b = C.make_batch(evam, 11, 64, 200, sizes=[(352, 198)] * 64)
    d = b.det
    thr = np.float32(b.threshold)
    assert (d[:, :, 2] == thr).any() and (d[:, :, 2] == np.nextafter(thr, np.float32(0))).any()
    term = d[:, :, 0] < 0
    assert (term[:, 0]).any() and (term[:, 1:].any(axis=1) & ~term[:, 0]).any()
    after = np.cumsum(term, axis=1) > 0
    assert (d[:, :, 2][after] >= thr).any()
    assert (d[:, :, 5] < d[:, :, 3]).any() and (d[:, :, 5] == d[:, :, 3]).any()
    assert (d[:, :, 3] < 0).any() and (d[:, :, 5] > 1).any()
    prod = d[:, :, 3].astype(np.float64) * 352
    assert ((prod - np.floor(prod)) == 0.5).any()
    want = C.python_rois(evam, b)
    got, count = C.host_rois(evam, b)
    assert count == len(want) > 100 and [tuple(r) for r in got.tolist()] == want


def test_half_products_round_up(evam):
    """x0 * W = q + .5 exactly: floor(q + .5 + .5) = q + 1, as the Python path (no fused multiply-add, no float32)."""
    det = np.zeros((1, 2, 7), np.float32)
    det[0, 0] = (0, 1, 0.9, 1 / 64, 1 / 4, 33 / 64, 3 / 4)   # 352 / 64 = 5.5, 198 / 4 = 49.5
    det[0, 1] = (0, 1, 0.9, 3 / 64, 0.0, 5 / 64, 1.0)
    b = C.Batch(det, [(352, 198)], None, C.TENSOR, 0.5, None)
    got, count = C.host_rois(evam, b)
    assert count == 2 and got.tolist() == [[0, 6, 50, 176, 99], [0, 17, 0, 11, 198]]
    assert [tuple(r) for r in got.tolist()] == C.python_rois(evam, b)


def test_cap_below_total(evam):
    b = C.make_batch(evam, 5, 8, 50, "mixed")
    want = C.python_rois(evam, b)
    assert len(want) > 20
    got, count = C.host_rois(evam, b, cap=7)
    assert count == len(want) and [tuple(r) for r in got.tolist()] == want[:7]


def test_label_list_and_threshold(evam):
    """An empty label list accepts nothing; the threshold is compared in float32, as numpy compares the float32 blob
    with a Python float."""
    b = C.make_batch(evam, 6, 4, 20)
    assert C.host_rois(evam, b._replace(labels=()))[1] == 0
    det = np.zeros((1, 3, 7), np.float32)
    det[0, :, 3:7] = (0.1, 0.1, 0.6, 0.6)
    det[0, :, 2] = (np.float32(0.3), np.nextafter(np.float32(0.3), np.float32(0)), np.nextafter(np.float32(0.3), np.float32(1)))
    b = C.Batch(det, [(64, 48)], None, C.TENSOR, 0.3, None)
    want = C.python_rois(evam, b)
    got, count = C.host_rois(evam, b)
    assert count == len(want) == 2 and [tuple(r) for r in got.tolist()] == want


def test_non_finite_rows_are_rejected(evam):
    det = np.zeros((1, 4, 7), np.float32)
    det[0, :, 2] = 0.9
    det[0, :, 3:7] = (0.1, 0.1, 0.6, 0.6)
    det[0, 0, 3] = np.nan
    det[0, 1, 6] = np.inf
    det[0, 2, 2] = np.nan
    got, count = C.host_rois(evam, C.Batch(det, [(64, 48)], None, C.TENSOR, 0.5, None))
    assert count == 1 and got.tolist() == [[0, 6, 5, 32, 24]]


def test_bad_arguments(evam):
    N = evam.native
    det = np.zeros((1, 1, 7), np.float32)
    with pytest.raises(evam.PreProcError) as e:
        N.ssd_rois_host(det, [(64, 48)], None, (0, 64), 0.5)
    assert e.value.status == N.ERR_INVALID_ARG
    with pytest.raises(evam.PreProcError) as e:
        N.ssd_rois_host(det, [(64, 48)], None, C.TENSOR, 0.5, cap=0)
    assert e.value.status == N.ERR_INVALID_ARG
    with pytest.raises(evam.PreProcError):
        N.ssd_rois_host(det, [(0, 48)], None, C.TENSOR, 0.5)
