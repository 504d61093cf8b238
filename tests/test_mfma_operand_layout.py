"""The slot tables of the MFMA phase-1 filter (csrc/knn_mfma.h: mf_candidate_operand, mf_query_operands) restated in numpy.

One v_mfma_f32_32x32x16_bf16 sums 16 products per (candidate, query) pair; the two operand builders must put the two factors
of every product of  d^2 - tau - slack = -2 p.q + |p|^2 + (|q|^2 - tau - slack)  into the SAME slot k, and the bf16 splits must
leave the sum within MF_SLACK of the exact value -- then the sign of the sum never clears a pair whose exact d^2 <= tau.
bf16 conversion is round-to-nearest-even on the uint32 view, the f32 accumulation is modelled in slot order and in reverse
(the order inside the matrix core is not documented).  No GPU."""
import itertools

import numpy as np

MF_SLACK = np.float32(1e-3)          # knn_mfma.h
BOX = np.array([2.25, 2.0, 2.0])     # |u_x| <= 2.25 (planned bricks), |u_y|, |u_z| <= 2: cell units about the brick centre
F = np.float32


def bf16(x):
    """f32 -> the nearest bf16 (ties to even), returned as f32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def fma(a, b, c):
    """f32 fused multiply-add: the product of two f32 is exact in f64; the sum is rounded once more going back to f32 (a double
    rounding in one case in 2^29, and then by one ulp of |p|^2: nothing below depends on it)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


# ---------------------------------------------------------------- the slot tables, by name
# k = 8 * (lane >> 5) + 0..7: k0..7 are built by lanes 0..31, k8..15 by lanes 32..63
CAND = ["ph_x", "ph_x", "pl_x", "ph_y", "pl_y", "ph_y", "1", "1",
        "ph_z", "ph_z", "pl_z", "n1", "n2", "n3", "1", "0"]
QUERY = ["-2qh_x", "-2ql_x", "-2qh_x", "-2qh_y", "-2qh_y", "-2ql_y", "s1", "s2",
         "-2qh_z", "-2ql_z", "-2qh_z", "1", "1", "1", "s3", "0"]


def candidate_pieces(u):
    """the named bf16 pieces of a candidate, each by its definition"""
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    out = {"1": np.ones(len(u), F), "0": np.zeros(len(u), F)}
    for c, v in zip("xyz", (ux, uy, uz)):
        out["ph_" + c] = bf16(v)
        out["pl_" + c] = bf16(v - out["ph_" + c])
    n = fma(uz, uz, fma(uy, uy, ux * ux))
    out["n1"] = bf16(n)
    out["n2"] = bf16(n - out["n1"])
    out["n3"] = bf16((n - out["n1"]) - out["n2"])
    return out


def query_pieces(u, s):
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    out = {"1": np.ones(len(u), F), "0": np.zeros(len(u), F)}
    for c, v in zip("xyz", (ux, uy, uz)):
        h = bf16(v)
        out["-2qh_" + c] = bf16(F(-2.0) * h)
        out["-2ql_" + c] = bf16(F(-2.0) * (v - h))
    out["s1"] = bf16(s)
    out["s2"] = bf16(s - out["s1"])
    out["s3"] = bf16((s - out["s1"]) - out["s2"])
    return out


# ---------------------------------------------------------------- the device's instruction sequences, statement by statement
def pk(lo, hi):
    """v_cvt_pk_bf16_f32: (lo -> bits 0..15, hi -> bits 16..31) as a pair of f32 values"""
    return bf16(lo), bf16(hi)


def mf_candidate_operand(u):
    """both half-waves run ONE sequence on selected inputs; returns the (N, 16) slots: columns 0..7 as lanes 0..31 build
    them, 8..15 as lanes 32..63 do"""
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    n = fma(uz, uz, fma(uy, uy, ux * ux))
    halves = []
    for upper in (False, True):
        a, b = (uz, n) if upper else (ux, uy)
        w0 = pk(a, a)
        la = a - w0[0]
        w1 = pk(la, b)
        rb = b - w1[1]
        t = pk(rb, rb)
        r2 = rb - t[0]
        w2 = pk(rb, r2 if upper else b)
        one, zero = np.ones(len(u), F), np.zeros(len(u), F)
        w3 = (one, zero) if upper else (one, one)
        halves.append(np.stack([*w0, *w1, *w2, *w3], axis=1))
    return np.concatenate(halves, axis=1)


def mf_query_operands(u, s):
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    hxf, hyf = pk(ux, uy)
    hzf = bf16(uz)
    lx, ly, lz = ux - hxf, uy - hyf, uz - hzf
    r1 = s - bf16(s)
    r2 = r1 - bf16(r1)
    m2, one, zero = F(-2.0), np.ones(len(u), F), np.zeros(len(u), F)
    lo = [pk(m2 * hxf, m2 * lx), pk(m2 * hxf, m2 * hyf), pk(m2 * hyf, m2 * ly), pk(s, r1)]
    up = [pk(m2 * hzf, m2 * lz), pk(m2 * hzf, one), (one, one), pk(r2, zero)]
    return np.stack([x for w in lo + up for x in w], axis=1)


def s_of(uq, tau):
    """|q|^2 - (tau (1 + 1e-6) + MF_SLACK) in the kernel's f32 statements (tau in cell units^2); -> (s, what was subtracted)"""
    nq2 = fma(uq[:, 2], uq[:, 2], fma(uq[:, 1], uq[:, 1], uq[:, 0] * uq[:, 0]))
    sub = tau * F(1.0 + 1e-6) + MF_SLACK
    return nq2 - sub, sub


def accumulate(prod, order):
    acc = np.zeros(len(prod), F)
    for k in order:
        acc = acc + prod[:, k]    # f32 + f32 -> f32
    return acc


# ---------------------------------------------------------------- the clouds
def _pairs():
    rng = np.random.default_rng(20251)
    n = 100_000
    p = (rng.uniform(-1.0, 1.0, (n, 3)) * BOX).astype(F)
    q = (rng.uniform(-1.0, 1.0, (n, 3)) * BOX).astype(F)
    corners = np.array(list(itertools.product(*[(-b, b) for b in BOX])), F)
    pc, qc = np.repeat(corners, 8, axis=0), np.tile(corners, (8, 1))
    p, q = np.concatenate([p, pc, pc]), np.concatenate([q, qc, qc])
    d2 = ((p.astype(np.float64) - q.astype(np.float64)) ** 2).sum(1)
    # tau: a third of the pairs anywhere in (0, 4] cell units^2 (the radius is one cell, 1.9 at most where it is widened), a
    # third ON the boundary -- the smallest f32 >= d^2, so that exact d^2 <= tau holds by less than an ulp -- and a third just
    # outside it (the largest f32 < d^2)
    tau = rng.uniform(0.05, 4.0, len(p)).astype(F)
    up = d2.astype(F)
    up = np.where(up.astype(np.float64) < d2, np.nextafter(up, F(np.inf)), up)
    dn = np.nextafter(up, F(-np.inf))
    dn = np.where(dn.astype(np.float64) >= d2, np.nextafter(dn, F(-np.inf)), dn)
    kind = np.arange(len(p)) % 3
    tau = np.where(kind == 1, up, np.where(kind == 2, np.maximum(dn, F(0.0)), tau)).astype(F)
    return p, q, tau, d2


def test_both_tables_address_the_same_product_in_every_slot():
    want = [("ph_" + c, "-2qh_" + c) for c in "xyz"] + [("ph_" + c, "-2ql_" + c) for c in "xyz"] + \
           [("pl_" + c, "-2qh_" + c) for c in "xyz"] + [("n%d" % i, "1") for i in (1, 2, 3)] + \
           [("1", "s%d" % i) for i in (1, 2, 3)] + [("0", "0")]
    assert sorted(zip(CAND, QUERY)) == sorted(want)
    # k0..7 need x and y only, k8..15 z and the norm only (what each half-wave builds), two s pieces below and one above
    assert not any(n.endswith("z") or n.startswith("n") for n in CAND[:8])
    assert not any(n.endswith(("x", "y")) for n in CAND[8:])
    assert sorted(QUERY[6:8] + QUERY[14:15]) == ["s1", "s2", "s3"]


def test_the_instruction_sequences_fill_the_slots_the_tables_name():
    p, q, tau, _ = _pairs()
    s, _ = s_of(q, tau)
    cp, qp = candidate_pieces(p), query_pieces(q, s)
    cs, qs = mf_candidate_operand(p), mf_query_operands(q, s)
    for k in range(16):
        assert np.array_equal(cs[:, k].view(np.uint32), cp[CAND[k]].view(np.uint32)), (k, CAND[k])
        assert np.array_equal(qs[:, k].view(np.uint32), qp[QUERY[k]].view(np.uint32)), (k, QUERY[k])
    # every slot IS a bf16 value, so the products are exact in f32
    for arr in (cs, qs):
        assert np.array_equal(arr.view(np.uint32) & 0xFFFF, np.zeros(arr.shape, np.uint32))


def test_the_sum_stays_within_the_slack_and_the_sign_never_clears_a_neighbour():
    p, q, tau, d2 = _pairs()
    s, sub = s_of(q, tau)
    prod64 = mf_candidate_operand(p).astype(np.float64) * mf_query_operands(q, s).astype(np.float64)
    prod = prod64.astype(F)
    assert np.array_equal(prod.astype(np.float64), prod64)     # bf16 x bf16 is exact in the f32 accumulator
    exact = d2 - sub.astype(np.float64)                        # float64 value of d^2 - tau - slack
    inside = d2 <= tau.astype(np.float64)
    assert inside.sum() > len(p) // 3 and (~inside).sum() > len(p) // 3
    worst = 0.0
    for order in (range(16), range(15, -1, -1)):
        acc = accumulate(prod, order)
        err = np.abs(acc.astype(np.float64) - exact)
        worst = max(worst, float(err.max()))
        assert err.max() < float(MF_SLACK), (err.max(), int(err.argmax()))
        # the predicate is the sign bit: a pair with exact d^2 <= tau must set it
        assert np.all(np.signbit(acc[inside])), int(np.count_nonzero(~np.signbit(acc[inside])))
    print("largest |sum - (d^2 - tau - slack)| = %.3g cell units^2 (header bound 3.8e-4, MF_SLACK 1e-3)" % worst)
    assert worst < 3.8e-4   # the bound the header comment derives


def test_a_dead_lane_passes_nothing():
    p, q, _, _ = _pairs()
    s = np.full(len(q), 1.0e30, F)   # tau < 0: a lane without a query
    prod = (mf_candidate_operand(p).astype(np.float64) * mf_query_operands(q, s).astype(np.float64)).astype(F)
    for order in (range(16), range(15, -1, -1)):
        assert not np.any(np.signbit(accumulate(prod, order)))
