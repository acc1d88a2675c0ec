"""numpy restatement of the matrix-core full pass of the split planes (kernels_scan42.h: u42_query_i16_kernel and the
epilogue of scan_u42_mfma_kernel), float32 arithmetic in the kernels' formulas.  Shared by
tests/test_selection_bounds_u42_mfma.py (CPU) and tests/test_gpu_u42_mfma.py."""
import numpy as np

F32, F64 = np.float32, np.float64
QMAX = 32512          # |Q_i| <= 127 * 256
MARK_HIGH, MARK_LOW = F32(2.0 ** 64), F32(2.0 ** -44)
MAX_DIMP = 384        # the largest instanced row (12 units)


def quantise_query(q):
    """q [dimp] fp32 -> dict(delta, Q, H, L int32 [dimp], e2, marked)"""
    q = np.asarray(q, F32)
    mx = F32(np.max(np.abs(q))) if np.isfinite(q).all() else F32(np.inf)
    marked = bool(not np.isfinite(q).all() or mx >= MARK_HIGH or (mx > 0 and mx < MARK_LOW))
    dimp = q.shape[0]
    if marked or mx == 0:
        z = np.zeros(dimp, np.int32)
        return dict(delta=F32(1), Q=z, H=z, L=z, e2=F32(0), marked=marked)
    e = int(np.floor(np.log2(F64(mx))))           # mx in [2^e, 2^(e + 1))
    delta = F32(2.0 ** (e - 14))
    if F32(mx / delta) > F32(QMAX):
        delta = F32(delta * F32(2))
    with np.errstate(over="ignore"):
        x = (q * F32(F32(1) / delta)).astype(F32)  # exact: a power of two
    r = np.rint(x).astype(F32)
    rho = (x - r).astype(F32)
    rr = (rho * rho).astype(F32).sum(dtype=F32)
    Q = r.astype(np.int32)
    H = (Q + 128) >> 8
    L = Q - 256 * H
    e2 = F32(delta * F32(np.sqrt(rr, dtype=F32) * F32(1.0005) + F32(1e-20)))
    return dict(delta=delta, Q=Q, H=H, L=L, e2=e2, marked=False)


def query_consts(q, qq):
    """the U42QConst of a query: dp, qsum305, qsum32, q2, round1' (u6_query_sums' sums in numpy's order)"""
    q = np.asarray(q, F32)
    dimp = q.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        ss = q.sum(dtype=F32)
        q1 = F32(np.abs(q).sum(dtype=F32) * F32(1.0 + 1e-5))
        q2 = F32(np.sqrt((q * q).astype(F32).sum(dtype=F32), dtype=F32) * F32(1.0 + 1e-5) + F32(1e-37))
        qsum32 = F32(F32(32) * ss)
        round1 = F32(F32(F32(6e-6) * F32(dimp + 8)) * q1 + F32(dimp) * F32(2.0 ** -138))
        qterm = F32(F32(F32(F32(60.0) * np.sqrt(F32(dimp), dtype=F32)) * qq["e2"]) * F32(1.0 + 1e-5))
        return dict(dp=F32(qq["delta"] * F32(2.0 ** -9)), qsum305=F32(F32(30.5) * F32(qsum32 * F32(0.03125))), qsum32=qsum32, q2=q2,
                    round1=F32(round1 + qterm))


def p_bits(h, Q, dp):
    """2^-9 P^ of every row, as the kernel's survivor entries carry it: float(P_int) * (2^-9 delta); also P_int (int64)"""
    p_int = h.astype(np.int64) @ Q.astype(np.int64)
    assert np.all(np.abs(p_int) < 2 ** 31)
    return (p_int.astype(np.int32).astype(F32) * dp).astype(F32), p_int


def first_stage(p4, s, a4, kc):
    """w4 = s (2048 p4 - 30.5 sum q) (2048 p4 is exact: one rounding in the difference) and m4' = fma(a4, |q|_2, s round1')"""
    with np.errstate(over="ignore", invalid="ignore"):
        w4 = (s * (F32(2048) * p4 - kc["qsum305"]).astype(F32)).astype(F32)
        m4 = (a4.astype(F64) * F64(kc["q2"]) + (s * kc["round1"]).astype(F32).astype(F64)).astype(F32)
    return w4, m4


def refine(p4, l, s, a6, q, kc):
    """w6 = s ((2048 p4 + sum l_i q_i) - 32 sum q) and m6' = fma(a6, |q|_2, s round1'); the remainders' sum in numpy's order"""
    with np.errstate(over="ignore", invalid="ignore"):
        qsum = (l.astype(F32) * np.asarray(q, F32)[None, :]).astype(F32).sum(axis=1, dtype=F32)
        w6 = (s * ((F32(2048) * p4.astype(F64) + qsum.astype(F64)).astype(F32) - kc["qsum32"]).astype(F32)).astype(F32)
        m6 = (a6.astype(F64) * F64(kc["q2"]) + (s * kc["round1"]).astype(F32).astype(F64)).astype(F32)
    return w6, m6
