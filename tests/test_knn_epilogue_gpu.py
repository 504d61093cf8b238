"""-m gpu: the float64 root and the numpy-order row means beneath every SOR mean distance, on bits.

The KNN kernels' results are (float)(sum of k float64 roots / k); the rest of the suite sees the root (sqrt_rn_dist2, a
hand-cut Goldschmidt sequence without range scaling) and the order of the additions (mean_from_net, mean_from_list,
pairwise_sum_le128, pairwise_sum_np in csrc/knn_common.h) only through that float32 on ordinary clouds, where a root one
ulp off or another order changes none of 200 000 results.  Here the same inline functions run through gsx_knn_probe_*_dev
(csrc/knn_probe.hip) on inputs made to fail: roots next to a rounding boundary in every binade a squared distance can lie
in, and rows whose float32 mean is decided by the order of the float64 additions (tests/epilogue_cases.py; what the
generator promises is asserted without a GPU in tests/test_epilogue_cases_host.py).  No tolerances anywhere."""
import numpy as np
import pytest

import epilogue_cases as ec

pytestmark = pytest.mark.gpu

CASES = ec.mean_cases()
FORM_NAMES = {ec.NET: "net", ec.LIST: "list", ec.LE128: "le128", ec.NP: "np"}


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def _roots_on_device(ctx, x, mode):
    d_in = ctx.alloc(x.nbytes).upload(x)
    d_out = ctx.alloc(x.nbytes)
    try:
        ctx.knn_probe_root(d_in.ptr, len(x), mode, d_out.ptr)
        return d_out.download(np.float64, len(x))
    finally:
        d_in.free()
        d_out.free()


def _assert_roots(x, got):
    want = np.sqrt(x)          # IEEE: correctly rounded
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, "%d of %d roots differ from np.sqrt; first: %s" % (
        len(bad), len(x), [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]])


def test_sqrt_rn_dist2_is_correctly_rounded_on_its_domain(ctx, lib):
    """sqrt_rn_dist2 (knn_brick's, knn_leaf's and knn_anyk's epilogue) == np.sqrt as uint64 on 0 and [2^-298, 2^260): both ends,
    every binade (2048 random mantissas, all zeros, all ones, 1 + ulp), 1024 near-ties per binade pair with their
    neighbours, the doubles whose root lies within 2^-42 ulp of a tie (without them the routine passes with its last
    correction step removed), exact squares -- 4.3M values, one launch"""
    x = ec.root_inputs()
    _assert_roots(x, _roots_on_device(ctx, x, lib.PROBE_ROOT_DIST2))


def test_dsqrt_rn_is_correctly_rounded(ctx, lib):
    """__dsqrt_rn (every other epilogue, the SPZ and compressed-PLY readers): the same inputs, and what lies outside
    sqrt_rn_dist2's domain -- subnormals, the smallest and largest binades, +inf"""
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 0x7FF0000000000000, 1 << 16, dtype=np.uint64)
    sub = rng.integers(1, 1 << 52, 1 << 12, dtype=np.uint64)
    edge = np.array([1, (1 << 52) - 1, 1 << 52, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000], np.uint64)
    x = np.concatenate([ec.root_inputs(), np.concatenate([wide, sub, edge]).view(np.float64)])
    _assert_roots(x, _roots_on_device(ctx, x, lib.PROBE_ROOT_DSQRT))


def _means_on_device(ctx, d2, k, form, cap):
    m, stride = d2.shape
    d_in = ctx.alloc(d2.nbytes).upload(d2)
    d_out = ctx.alloc(4 * m)
    try:
        ctx.knn_probe_mean(d_in.ptr, m, stride, k, form, cap, d_out.ptr)
        return d_out.download(np.float32, m)
    finally:
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("form,cap,k", CASES, ids=["%s%s-k%d" % (FORM_NAMES[f], cap or "", k) for f, cap, k in CASES])
def test_row_means_in_numpy_order(ctx, form, cap, k):
    """every form of the epilogue at the k that select it, against the reference's own expression evaluated by numpy
    (epilogue_cases.reference_means), on rows where another order of the additions gives another float32: rows led by
    duplicate points, rows whose last root dominates and rows whose roots are all of one size, 64 different ones per block,
    each with two further neighbours behind its k entries that no sum may read"""
    r = ec.rows_for_k(k)
    got = _means_on_device(ctx, r["d2"], k, form, cap)
    want = r["want"]
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        b = np.sqrt(r["d2"][:, :k])
        like = [f.__name__ for f in ec.OTHER_ORDERS + (ec.sum_eight_no_tail,)
                if (ec.mean_f32(f(b), k).view(np.uint32)[bad] == got.view(np.uint32)[bad]).all()]
        pytest.fail("%d of %d rows differ (%d of them rows that tell orders apart); first rows %s: got %s want %s; every "
                    "differing row equals: %s" % (len(bad), len(want), int(r["kept"][bad].sum()), bad[:4].tolist(),
                                                  got[bad[:4]].tolist(), want[bad[:4]].tolist(), like or "no other order tried"))


def test_probe_refuses_what_no_kernel_instantiates(ctx, lib):
    d2 = np.sort(np.random.default_rng(0).random((4, 80)), axis=1)
    d_in = ctx.alloc(d2.nbytes).upload(d2)
    d_out = ctx.alloc(64)
    try:
        for form, cap, k, msg in ((ec.NET, 60, 60, "TopNet<60>"), (ec.NET, 10, 8, "TopNet<10>"), (ec.NET, 8, 9, "does not fit"),
                                  (ec.LIST, 13, 8, "TopList<13>"), (ec.LIST, 9, 9, "does not fit"), (4, 0, 8, "unknown form"),
                                  (ec.LE128, 0, 129, "k <= 128"), (ec.NP, 0, 1001, "k <= 1000"), (ec.NET, 8, 0, "1 <= k")):
            with pytest.raises(lib.GsxError, match=msg):
                ctx.knn_probe_mean(d_in.ptr, 4, 2000 if k > 80 else 80, k, form, cap, d_out.ptr)
        with pytest.raises(lib.GsxError, match="unknown mode"):
            ctx.knn_probe_root(d_in.ptr, 4, 2, d_in.ptr)
    finally:
        d_in.free()
        d_out.free()
