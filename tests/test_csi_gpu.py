"""RI / PMI / SINR selection on the GPU (csi_kernel.hip through srsran_precoding_pmi_select, srsran_precoding_cn,
srsran_ue_dl_gpu_csi_batch) against the reference's own functions compiled into oracle/_ref/libsrsref.so: the
dispatching srsran_precoding_pmi_select (its AVX2 build runs the _simd forms, whose sample set the kernel uses; the
_gen forms sample other points and differ by up to 4e-3) and srsran_precoding_cn.

Channels: a fixed complex 2 x 2 matrix with 5 % ripple per RE, nof_symbols in {192, 1008, 2520} x noise in
{0.01, 0.3}, one of 16800 symbols, one with noise 0 (the noise bound of precoding.c:2781-2783).

Tolerances (DESIGN.md, section "Channel-state feedback"): sinr_1l 1e-5 relative (no rcp in it; a sum of at most ~700
float terms of one sign).  sinr_2l and cn: the largest difference, over exactly these cases, between restate_simd /
restate_cn below (float32, exact division, numpy's pairwise sums) and the compiled reference, measured on the build
machine, times 4 (GPU summation order and FMA contraction add float rounding on top of the reference's rcp):
  sinr_2l  measured 1.468e-4 relative (n192_noise0.3; 1.9e-5 .. 1.5e-4 over the cases)  -> TOL_2L = 5.9e-4
  cn       measured 2.861e-6 dB (0 .. 2.9e-6 over the cases)                           -> TOL_CN = 1.14e-5 dB
(sinr_1l of the restatement is within 2.2e-7 of the reference.)
Decisions (pmi_1l, pmi_2l, ri_cn, select_ri_pmi's ri / pmi restated over the reference's SINRs) must be equal; every
case's margins (best against second-best SINR, |cn - 17|, the 0.1 dB and 20 dB thresholds) are asserted to exceed ten
times the tolerance, so a seed that does not qualify fails loudly."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

TOL_1L = 1e-5
MEAS_2L, MEAS_CN = 1.468e-4, 2.861e-6  # measured: see the module docstring
TOL_2L, TOL_CN = 4 * MEAS_2L, 4 * MEAS_CN

CASES = [  # (nof_symbols, noise, seed)
    (192, 0.01, 1), (192, 0.3, 2), (1008, 0.01, 3), (1008, 0.3, 4), (2520, 0.01, 5), (2520, 0.3, 6),
    (16800, 0.3, 7), (1008, 0.0, 8),
]
IDS = [f"n{c[0]}_noise{c[1]}" for c in CASES]


def channel(seed, n, ripple=0.05):
    """h[port][rx] (2, 2, n) complex64: a fixed matrix, every RE with its own 5 % ripple"""
    rng = np.random.default_rng(seed)
    H = (rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))) / np.sqrt(2)
    w = (rng.standard_normal((2, 2, n)) + 1j * rng.standard_normal((2, 2, n))) / np.sqrt(2)
    return (H[:, :, None] * (1 + ripple * w)).astype(np.complex64)


def bound_noise(noise):
    noise = f32(noise)
    return f32(1e-9) if not (noise >= f32(1e-9) and np.isfinite(noise)) else noise


def _tree8(g):
    """(nblk, 8) -> the hadd tree of one SIMD block"""
    a = g[:, 0::2] + g[:, 1::2]
    b = a[:, 0::2] + a[:, 1::2]
    return b[:, 0] + b[:, 1]


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def restate_simd(h, noise):
    """srsran_precoding_pmi_select_1l_simd / _2l_simd (precoding.c:2350-2465, 2595-2745) in float32 with exact
    division, on the SIMD sample set -> (sinr_1l[4], sinr_2l[2])"""
    n = h.shape[2]
    nblk = n // 192
    idx = 24 * np.arange(8 * nblk)
    noise = bound_noise(noise)
    ri = lambda z: (z.real.astype(f32), z.imag.astype(f32))  # noqa: E731
    h00, h01, h10, h11 = ri(h[0, 0, idx]), ri(h[1, 0, idx]), ri(h[0, 1, idx]), ri(h[1, 1, idx])
    conj = lambda z: (z[0], -z[1])  # noqa: E731
    mulj = lambda z: (-z[1], z[0])  # noqa: E731
    add = lambda a, b: (a[0] + b[0], a[1] + b[1])  # noqa: E731
    sub = lambda a, b: (a[0] - b[0], a[1] - b[1])  # noqa: E731
    b0, b1 = [], []
    for i in range(4):
        t0, t1 = (conj(h01), conj(h11)) if i < 2 else (mulj(conj(h01)), mulj(conj(h11)))
        op = add if i in (0, 3) else sub
        a0, a1 = op(conj(h00), t0), op(conj(h10), t1)
        b0.append(add(_cmul(a0, h00), _cmul(a1, h10)))
        b1.append(add(_cmul(a0, h01), _cmul(a1, h11)))
    re_c = [b0[0][0] + b1[0][0], b0[1][0] - b1[1][0], b0[2][0] - b1[2][1], b0[3][0] + b1[3][1]]
    count = f32(nblk)
    s1 = [np.sum(_tree8((c * f32(0.5)).reshape(nblk, 8)) / f32(8), dtype=f32) / (noise * count) for c in re_c]
    s2 = []
    for i0, i1, rot in ((0, 1, False), (2, 3, True)):
        q0, q1 = (mulj(b1[i0]), mulj(b1[i1])) if rot else (b1[i0], b1[i1])
        c00, c01 = add(b0[i0], q0), sub(b0[i0], q0)
        c10, c11 = add(b0[i1], q1), sub(b0[i1], q1)
        c00, c01, c10, c11 = [(c[0] * f32(0.25), c[1] * f32(0.25)) for c in (c00, c01, c10, c11)]
        c00 = (c00[0] + noise, c00[1])
        c11 = (c11[0] + noise, c11[1])
        det = _cmul(c00, c11)[0] - _cmul(c01, c10)[0]
        det = np.where(det < f32(1e-10), f32(1e-10), det)
        inv = noise * (f32(1) / det)
        g0 = f32(1) / (c00[0] * inv) - f32(1)
        g1 = f32(1) / (c11[0] * inv) - f32(1)
        g0 = np.where(g0 < f32(1e-9), f32(1e-9), g0)
        g1 = np.where(g1 < f32(1e-9), f32(1e-9), g1)
        blk = (_tree8(g0.reshape(nblk, 8)) + _tree8(g1.reshape(nblk, 8))) / f32(8)
        s2.append(np.sum(blk, dtype=f32) / count)
    return np.array(s1, f32), np.array(s2, f32)


def restate_cn(h):
    """srsran_precoding_2x2_cn_gen + srsran_mat_2x2_cn (precoding.c:2798-2822, mat.c:128-160) in float32 on every
    24th index; samples with NaN / Inf eigenvalues skipped -> (cn in dB, samples counted)"""
    idx = np.arange(0, h.shape[2], 24)
    x = lambda z: z.real.astype(f32)  # noqa: E731
    y = lambda z: z.imag.astype(f32)  # noqa: E731
    h00, h01, h10, h11 = h[0, 0, idx], h[1, 0, idx], h[0, 1, idx], h[1, 1, idx]
    with np.errstate(invalid="ignore"):
        a00 = x(h00) * x(h00) + x(h01) * x(h01) + y(h00) * y(h00) + y(h01) * y(h01)
        a11 = x(h10) * x(h10) + x(h11) * x(h11) + y(h10) * y(h10) + y(h11) * y(h11)
        a01 = (h00 * np.conj(h10) + h01 * np.conj(h11)).astype(np.complex64)
        b = a00 + a11
        c = a00 * a11 - (x(a01) * x(a01) + y(a01) * y(a01))
        sqr = np.sqrt(b * b - f32(4) * c)
        xmax, xmin = b + sqr, b - sqr
        ok = np.isfinite(xmax) & np.isfinite(xmin)
        cn = f32(10) * np.log10(np.minimum(xmax[ok], f32(1e9)) / np.maximum(xmin[ok], f32(1e-9)))
    return (np.sum(cn, dtype=f32) / f32(len(cn)) if len(cn) else f32(0)), int(ok.sum())


def db(x):
    with np.errstate(divide="ignore"):
        return f32(10) * np.log10(f32(x))


def select_ri_pmi(s1, p1, s2, p2):
    """select_ri_pmi (ue_dl.c:778-822) over SINR lists and their best entries -> (ri, pmi, sinr_db)"""
    best_db, ri, pmi = f32(-np.inf), 0, 0
    for this_ri, (s, p) in enumerate(((s1, p1), (s2, p2))):
        d = db(s[p])
        if float(d) > float(best_db) + 0.1 or d > f32(20.0):
            best_db, ri, pmi = d, this_ri, p
    return ri, pmi, best_db


def first_max(s):
    best, p = f32(0), 0
    for i, v in enumerate(s):
        if v > best:
            best, p = v, i
    return p


class Ref:
    """srsran_precoding_pmi_select / srsran_precoding_cn of the compiled reference"""

    def __init__(self):
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        if not O.ref_available():
            pytest.fail("oracle/_ref/libsrsref.so missing: the reference checker of this module was not built")
        L = ctypes.CDLL(O.REF_SO, mode=os.RTLD_LAZY)
        L.srsran_precoding_pmi_select.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)]
        L.srsran_precoding_pmi_select.restype = ctypes.c_int
        L.srsran_precoding_cn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.POINTER(ctypes.c_float)]
        L.srsran_precoding_cn.restype = ctypes.c_int
        self.L = L

    @staticmethod
    def _ptrs(h):
        rows = [[np.ascontiguousarray(h[p, r], np.complex64) for r in range(2)] for p in range(2)]
        ptrs = ((ctypes.c_void_p * 4) * 4)()
        for p in range(2):
            for r in range(2):
                ptrs[p][r] = rows[p][r].ctypes.data
        return ptrs, rows

    def pmi_select(self, h, noise, nl):
        ptrs, keep = self._ptrs(h)
        pmi, sinr = ctypes.c_uint32(0), (ctypes.c_float * 4)()
        n = self.L.srsran_precoding_pmi_select(ctypes.addressof(ptrs), h.shape[2], noise, nl, ctypes.byref(pmi), sinr)
        assert n == (4 if nl == 1 else 2)
        return pmi.value, np.array([sinr[i] for i in range(n)], f32)

    def cn(self, h):
        ptrs, keep = self._ptrs(h)
        cn = ctypes.c_float(0)
        assert self.L.srsran_precoding_cn(ctypes.addressof(ptrs), 2, 2, h.shape[2], ctypes.byref(cn)) == 0
        return f32(cn.value)


@pytest.fixture(scope="module")
def env():
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    ref = Ref()
    refs = {}
    for n, noise, seed in CASES:  # the reference's values of every case, computed once
        h = channel(seed, n)
        p1, s1 = ref.pmi_select(h, noise, 1)
        p2, s2 = ref.pmi_select(h, noise, 2)
        refs[(n, noise, seed)] = (h, p1, s1, p2, s2, ref.cn(h))
    from srsran_4g_amd import ue_dl as U
    import torch
    return U, torch, refs


def rel(a, b):
    return np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.abs(b.astype(np.float64)))


def margins_ok(s1, s2, cn):
    """the reference's own margins against ten times the tolerances"""
    def gap(s):
        o = np.sort(s.astype(np.float64))[::-1]
        return (o[0] - o[1]) / o[0]
    tol_db = 10 * np.log10(1 + max(TOL_1L, TOL_2L))
    d1, d2 = float(db(s1.max())), float(db(s2.max()))
    return {"pmi_1l": gap(s1) > 10 * TOL_1L, "pmi_2l": gap(s2) > 10 * TOL_2L, "ri_cn": abs(float(cn) - 17) > 10 * TOL_CN,
            "0.1 dB": abs(d2 - d1 - 0.1) > 10 * tol_db, "20 dB": abs(d2 - 20) > 10 * tol_db and abs(d1 - 20) > 10 * tol_db}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sinr_cn_and_decisions_match_reference(env, case):
    U, torch, refs = env
    n, noise, seed = case
    h, p1, s1, p2, s2, cn = refs[case]
    ok = margins_ok(s1, s2, cn)
    assert all(ok.values()), f"seed {seed} does not qualify: {ok}"
    r1, g_p1, g_s1 = U.precoding_pmi_select(h, noise, 1)
    r2, g_p2, g_s2 = U.precoding_pmi_select(h, noise, 2)
    rc, g_cn = U.precoding_cn(h)
    assert (r1, r2, rc) == (4, 2, 0)
    g_s1, g_s2 = np.array(g_s1, f32), np.array(g_s2, f32)
    print(f"\n{case}: sinr_1l rel {rel(g_s1, s1):.3g}, sinr_2l rel {rel(g_s2, s2):.3g}, cn diff "
          f"{abs(float(g_cn) - float(cn)):.3g} dB")
    assert rel(g_s1, s1) <= TOL_1L
    assert rel(g_s2, s2) <= TOL_2L
    assert abs(float(g_cn) - float(cn)) <= TOL_CN
    assert (g_p1, g_p2) == (p1, p2) == (first_max(s1), first_max(s2))
    assert int(g_cn < 17) == int(cn < 17)
    # the whole record in one call: the same kernel, so the same bits, and select_ri_pmi's rule on top
    ret, rec = U.precoding_csi_2x2(h, noise)
    assert ret == 0
    assert np.array_equal(rec["sinr_1l"], g_s1) and np.array_equal(rec["sinr_2l"], g_s2) and rec["cn"] == g_cn
    assert (int(rec["pmi_1l"]), int(rec["pmi_2l"]), int(rec["ri_cn"])) == (p1, p2, int(cn < 17))
    want = select_ri_pmi(s1, p1, s2, p2)
    assert (int(rec["ri"]), int(rec["pmi"])) == want[:2]
    assert abs(float(rec["sinr_db"]) - float(want[2])) <= 10 * np.log10(1 + max(TOL_1L, TOL_2L)) + 1e-5
    assert int(rec["cn_count"]) == (n + 23) // 24


def test_noise_bound(env):
    """noise 0, NaN, negative and subnormal all count as 1e-9 (precoding.c:2781-2783): one record, bit for bit"""
    U, torch, refs = env
    h = channel(8, 1008)
    recs = [U.precoding_csi_2x2(h, x)[1] for x in (1e-9, 0.0, float("nan"), -1.0, 1e-40, float("inf"))]
    for r in recs[1:]:
        assert r.tobytes() == recs[0].tobytes()


def test_host_rows_scratch_regrowth_is_bit_identical(env):
    """the process-wide scratch of the host-row calls: the smallest sample set, a larger one (the scratch is
    reallocated), the smallest again -- the two small records are the same bytes, and so are the two large ones"""
    U, torch, refs = env
    small, large = channel(21, 192), channel(22, 16800 + 2400)
    recs = [U.precoding_csi_2x2(h, 0.05) for h in (small, large, small, large)]
    assert all(r[0] == 0 for r in recs)
    assert recs[0][1].tobytes() == recs[2][1].tobytes() and recs[1][1].tobytes() == recs[3][1].tobytes()
    assert recs[0][1].tobytes() != recs[1][1].tobytes()


def test_rank_deficient_channel(env):
    """both ports' columns equal: ri_cn = 0 and every output finite"""
    U, torch, refs = env
    h = channel(21, 1008)
    h[1] = h[0]
    ret, rec = U.precoding_csi_2x2(h, 0.05)
    assert ret == 0 and int(rec["ri_cn"]) == 0 and rec["cn"] > 17
    assert np.all(np.isfinite(rec["sinr_1l"])) and np.all(np.isfinite(rec["sinr_2l"]))
    assert np.isfinite(rec["cn"]) and np.isfinite(rec["sinr_db"])


def test_nan_sample_is_skipped_by_cn(env):
    """a NaN estimate at index 984, which only the condition number samples (the SINR set of 1008 symbols ends at
    24 x 39): that sample is skipped and not counted (mat.c:146-149), cn is the mean of the other 41, the SINRs are
    those of the clean channel"""
    U, torch, refs = env
    case = CASES[3]
    h = refs[case][0].copy()
    clean = U.precoding_csi_2x2(h, case[1])[1]
    h[0, 0, 984] = np.nan
    ret, rec = U.precoding_csi_2x2(h, case[1])
    want_cn, want_count = restate_cn(h)
    assert ret == 0 and want_count == 41 and int(rec["cn_count"]) == 41 and int(clean["cn_count"]) == 42
    assert abs(float(rec["cn"]) - float(want_cn)) <= TOL_CN
    assert rec["cn"] != clean["cn"]
    assert np.array_equal(rec["sinr_1l"], clean["sinr_1l"]) and np.array_equal(rec["sinr_2l"], clean["sinr_2l"])


def test_host_call_refusals(env):
    U, torch, refs = env
    h = channel(1, 192)
    assert U.precoding_pmi_select(h, 0.1, 1, nof_symbols=191)[0] == -2  # SRSRAN_ERROR_INVALID_INPUTS
    assert U.precoding_pmi_select(h, 0.1, 3)[0] == -2
    assert U.precoding_cn(h, 4, 2)[0] == -1 and U.precoding_cn(h, 2, 1)[0] == -1  # SRSRAN_ERROR, as the reference


@pytest.mark.parametrize("alg", ["average", "interpolate"])
def test_csi_batch_equals_host_calls_on_the_batch_estimates(env, alg):
    """a 3-subframe srsran_ue_dl_gpu_decode_batch at 6 PRB, 2 ports x 2 rx, with the AVERAGE (one estimate row, read
    at j mod 72) and the INTERPOLATE (full grid) estimator: the records of srsran_ue_dl_gpu_csi_batch equal, bit
    for bit, what the host-pointer call returns for the batch's estimates and noise copied back"""
    U, torch, refs = env
    from srsran_4g_amd import sch
    from srsran_4g_amd.sch import _memcpy_d2h
    from synth import synth as S
    nprb, cell_id, tbs, Qm = 6, 17, 1544, 4
    U.use_standard_symbol_size(True)
    ue = U.UeDl(U.cell(nprb, 2, cell_id), 2)
    ue.cfg.chest_cfg.estimator_alg = 1 if alg == "interpolate" else 0
    rng = np.random.default_rng(3)
    xs, sfs, keep = [], [], []
    d_pl = torch.zeros((3, 2, tbs // 8 + 64), dtype=torch.uint8, device="cuda")
    for b, tti in enumerate((1, 2, 3)):
        pls = [rng.integers(0, 256, tbs // 8, dtype=np.uint8) for _ in range(2)]
        x, nre = S.pdsch_subframe(nprb, cell_id, 2, tti, 1, 0x1234, tbs, Qm, 0, pls, snr_db=25.0 - 5 * b, rng=rng)
        sbs = [sch.SoftbufferRx(nof_prb=nprb) for _ in range(2)]
        cfg = U.pdsch_cfg(nprb, nre, (tbs, tbs), (Qm, Qm), softbuffers=sbs)
        keep += [sbs, cfg]
        xs.append(x)
        sfs.append((tti, 1, cfg, [d_pl[b, 0].data_ptr(), d_pl[b, 1].data_ptr()], [1, 1]))
    d_x = torch.from_numpy(np.stack(xs).view(np.float32)).cuda()
    d_res = torch.full((6,), 7, dtype=torch.int32, device="cuda")
    d_avg = torch.zeros(6, dtype=torch.float32, device="cuda")
    d_csi = torch.zeros(3 * 64, dtype=torch.uint8, device="cuda")
    try:
        assert ue.gpu_decode_batch(sfs, d_x.data_ptr(), d_res.data_ptr(), d_avg.data_ptr(), 0.0, None) == 6
        assert ue.csi_batch(3, d_csi.data_ptr()) == 0
        torch.cuda.synchronize()
        got = d_csi.cpu().numpy().view(U.CSI_DTYPE)
        n = 14 * 12 * nprb
        for b in range(3):
            d_ce, row_len, d_noise = ue.last_ce(b)
            assert row_len == (n if alg == "interpolate" else 12 * nprb)
            ce = torch.empty(4 * row_len * 2, dtype=torch.float32)
            noise = torch.empty(1, dtype=torch.float32)
            _memcpy_d2h(ce, d_ce, ce.numel() * 4)
            _memcpy_d2h(noise, d_noise, 4)
            rows = ce.numpy().view(np.complex64).reshape(2, 2, row_len)
            h = rows[:, :, np.arange(n) % row_len]  # index j of the one-row form reads row[j mod 12 nof_prb]
            ret, want = U.precoding_csi_2x2(h, float(noise[0]))
            assert ret == 0 and np.isfinite(want["cn"]) and want["sinr_1l"].max() > 0
            assert got[b].tobytes() == want.tobytes(), (b, got[b], want)
        assert ue.csi_batch(4, d_csi.data_ptr()) == -2  # more subframes than the batch left
    finally:
        ue.free()
        for k in keep:
            if isinstance(k, list):
                for sb in k:
                    sb.free()


def test_ue_shape_refusals(env):
    """fewer than 2 ports: SRSRAN_SUCCESS and nothing written; 2 ports x 1 rx: SRSRAN_ERROR"""
    U, torch, refs = env
    ue = U.UeDl(U.cell(6, 1, 3), 2)
    try:
        ri, cn = ctypes.c_uint32(77), ctypes.c_float(-5.0)
        assert U.lib().srsran_ue_dl_select_ri(ctypes.byref(ue.q), ctypes.byref(ri), ctypes.byref(cn)) == 0
        assert (ri.value, cn.value) == (77, -5.0)
        assert ue.select_ri_pmi()[0] == 0 and ue.csi_batch(1, None) == 0
    finally:
        ue.free()
    ue = U.UeDl(U.cell(6, 2, 3), 1)
    try:
        assert ue.select_ri()[0] == -1 and ue.select_ri_pmi()[0] == -1 and ue.csi_batch(1, None) == -1
    finally:
        ue.free()
