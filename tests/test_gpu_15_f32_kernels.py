"""The exact-fp32 kernels one by one against float64 (a-V: vocoder, mel / STFT front end, ECAPA prosody
encoder, MDX-Net TDF layers, the K = 100 input projection, the AdaLN tables).  Every comparison is per element against a DERIVED bound
(tests/f32_tolerance.py states each derivation; tests/test_f32_kernel_tolerance_cpu.py shows each bound rejects a plausible bug), and
every output buffer carries NaN canaries around what the kernel may write."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import f32_tolerance as TOL
from f32_tolerance import U, check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS: dict = {}           # worst error / bound per kernel, printed by test_zz_report (run with -s to see it)

F32_BIAS, F32_GELU, F32_SILU, F32_RES_SCALE, F32_ADD2, F32_RELU, F32_SIGMOID, F32_ROWAFF_RELU, F32_ROWAFF_RELU_RES = range(9)
ACT = {F32_BIAS: "bias", F32_GELU: "gelu", F32_SILU: "silu", F32_RES_SCALE: "bias", F32_ADD2: "bias", F32_RELU: "relu",
       F32_SIGMOID: "sigmoid", F32_ROWAFF_RELU: "relu", F32_ROWAFF_RELU_RES: "relu"}


def _lib():
    from lemas_tts_amd import _lib as L
    return L, L.testlib()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def nan_buf(n: int) -> torch.Tensor:
    return torch.full((n,), float("nan"), device=DEV)


def act_ref(act: str, z: np.ndarray) -> np.ndarray:
    t = torch.from_numpy(z)
    if act == "gelu":
        return torch.nn.functional.gelu(t).numpy()
    if act == "silu":
        return torch.nn.functional.silu(t).numpy()
    if act == "sigmoid":
        return torch.sigmoid(t).numpy()
    if act == "relu":
        return np.maximum(z, 0.0)
    return z


def f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def tile_height(M: int, N: int, nbatch: int = 0) -> int:
    """gemm_f32.hip launch(): 32-row tiles for M <= 32 or fewer than 400 64-row workgroups"""
    g64 = math.ceil(N / 64) * math.ceil(M / 64) * max(nbatch, 1)
    return 32 if M <= 32 or g64 < 400 else 64


# ---- gemm_f32 --------------------------------------------------------------------------------------------------------------------
def run_gemm(epi, M, N, K, *, seed=0, lda=None, ldw=None, ldc=None, out_off=0, add_off=0, with_bias=True, with_colscale=True,
             ldres=None, rowmask=None, rowaff=True, rows_per_ch=3, nch=5, inplace_res=False, key=None):
    """one launch through lemas_k_gemm_f32_ex with NaN canaries in every padding column and in the rows past the written ones"""
    L, lib = _lib()
    rng = np.random.default_rng(seed * 7919 + epi * 131 + M * 17 + N * 3 + K)
    lda, ldw, ldc = lda or K, ldw or K, ldc or N
    rows = 2 * M if epi == F32_ADD2 else M
    A = np.full((M, lda), np.nan, np.float32)
    A[:, :K] = f32(rng, M, K)
    Wm = np.full((N, ldw), np.nan, np.float32)           # NaN in the padding: a read past K would poison the result
    Wm[:, :K] = f32(rng, N, K, scale=1.0 / math.sqrt(K))
    bias = f32(rng, N) if with_bias else None
    a = L.GemmF32Args()
    Ad, Wd = dev(A), dev(Wm)
    keep = [Ad, Wd]
    a.A, a.lda, a.W, a.ldw, a.M, a.N, a.K = Ad.data_ptr(), lda, Wd.data_ptr(), ldw, M, N, K
    if bias is not None:
        bd = dev(bias); keep.append(bd); a.bias = bd.data_ptr()
    extra = 3                                                 # canary rows after the last written one
    outbuf = nan_buf(out_off + (rows + extra) * ldc)
    a.out, a.ldc = outbuf.data_ptr() + 4 * out_off, ldc
    A64, W64 = A[:, :K].astype(np.float64), Wm[:, :K].astype(np.float64)
    b64 = bias.astype(np.float64) if bias is not None else np.zeros(N)
    z = A64 @ W64.T + b64
    accb = TOL.gemm_acc_bound(A64, W64, b64 if bias is not None else None, K)
    act = ACT[epi]
    inner = None
    scale = 1.0
    if epi == F32_RES_SCALE:
        ldres = ldres or ldc
        res = f32(rng, M, ldres)
        rd = dev(res); keep.append(rd); a.res, a.ldres = rd.data_ptr(), ldres
        cs = (rng.uniform(0.25, 2.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32) if with_colscale else np.ones(N, np.float32)
        if with_colscale:
            cd = dev(cs); keep.append(cd); a.colscale = cd.data_ptr()
        inner = cs * z
        ref = res[:, :N].astype(np.float64) + inner
        scale = cs[None, :].astype(np.float64)
    elif epi in (F32_ROWAFF_RELU, F32_ROWAFF_RELU_RES):
        ch = (np.arange(M) // rows_per_ch) % nch
        if rowaff:
            rs = (rng.uniform(0.25, 2.0, nch) * rng.choice([-1.0, 1.0], nch)).astype(np.float32)
            rh = f32(rng, nch)
            sd, hd = dev(rs), dev(rh); keep += [sd, hd]
            a.rowscale, a.rowshift = sd.data_ptr(), hd.data_ptr()
        else:
            rs, rh = np.ones(nch, np.float32), np.zeros(nch, np.float32)
        a.rows_per_ch, a.nch = rows_per_ch, nch
        scale = rs[ch].astype(np.float64)[:, None]
        inner = scale * z + rh[ch].astype(np.float64)[:, None]
        ref = np.maximum(inner, 0.0)
        if epi == F32_ROWAFF_RELU_RES:
            if inplace_res:                               # res == out: each element read and written by one thread
                res = f32(rng, M, ldc)
                res[:, N:] = np.nan
                body = torch.from_numpy(res.reshape(-1)).to(DEV)
                outbuf[out_off:out_off + M * ldc] = body
                a.res, a.ldres = a.out, ldc
            else:
                ldres = ldres or ldc
                res = f32(rng, M, ldres)
                rd = dev(res); keep.append(rd); a.res, a.ldres = rd.data_ptr(), ldres
            ref = ref + res[:, :N].astype(np.float64)
    elif epi == F32_ADD2:
        addbuf = nan_buf(add_off + 2 * M * ldc)
        addv = f32(rng, 2 * M, ldc)
        addv[:, N:] = np.nan                               # the add operand's padding is never read either
        addbuf[add_off:] = torch.from_numpy(addv.reshape(-1)).to(DEV)
        keep.append(addbuf)
        a.add = addbuf.data_ptr() + 4 * add_off
        zz = np.concatenate([z, z])
        ref = zz + addv[:, :N].astype(np.float64)
        z, accb = zz, np.concatenate([accb, accb])
    else:
        ref = act_ref(act, z)
    if rowmask is not None:
        md = torch.from_numpy(rowmask.astype(np.uint8)).to(DEV); keep.append(md)
        a.rowmask = md.data_ptr()
        if epi != F32_ADD2:                               # ADD2 ignores the mask by design (both CFG rows are always written)
            ref = ref.copy()
            ref[rowmask.astype(bool)] = 0.0
    rc = lib.lemas_k_gemm_f32_ex(epi, C.byref(a), None)
    L.check(rc, f"gemm_f32_ex epi {epi} M {M} N {N} K {K}")
    flat = outbuf.cpu().numpy()
    assert np.isnan(flat[:out_off]).all(), "wrote before out"
    o = flat[out_off:].reshape(rows + extra, ldc)
    assert np.isnan(o[rows:]).all(), "wrote past the last row"
    if ldc > N:
        assert np.isnan(o[:rows, N:]).all(), "wrote into the padding columns N .. ldc - 1"
    bound = TOL.gemm_bound(accb, z, ref, act, scale=scale, inner=inner)
    if rowmask is not None and epi != F32_ADD2:
        bound = np.where(rowmask.astype(bool)[:, None], 0.0, bound)
    check(o[:rows, :N], ref, bound, f"gemm_f32 epi {epi} M {M} N {N} K {K}", RATIOS, key or "gemm_f32")
    return o[:rows, :N]


EPIS = list(range(9))
NK_SMALL = [(1, 4), (3, 28), (4, 32), (65, 36), (100, 100), (1026, 132), (65, 1024), (4, 1024)]


@pytest.mark.parametrize("M", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("epi", EPIS)
def test_gemm_f32_epilogue_small(epi, M):
    """every epilogue at every tile edge: K one tile, a partial tile, an odd / even tile count, a tail inside a tile (28, 36, 100, 132)"""
    assert tile_height(M, 1026) == 32
    for N, K in NK_SMALL:
        run_gemm(epi, M, N, K)


@pytest.mark.parametrize("M,tile", [(1536, 32), (1600, 64)])
@pytest.mark.parametrize("epi", EPIS)
def test_gemm_f32_epilogue_tile_switch(epi, M, tile):
    """1536 x 1024 is 384 64-row workgroups (-> the 32-row tile), 1600 x 1024 is 400 (-> the 64-row tile)"""
    assert tile_height(M, 1024) == tile
    run_gemm(epi, M, 1024, 100)
    if epi == F32_BIAS:
        run_gemm(epi, M, 1024, 1024)


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(33, 65, 36), (65, 100, 132), (1600, 70, 100)])
def test_gemm_f32_strides_and_scalar_store(epi, M, N, K):
    """lda / ldw / ldc beyond the extent; ldc % 4 != 0 and out / add one float off 16 B (the scalar store); canaries in the padding"""
    run_gemm(epi, M, N, K, lda=K + 8, ldw=K + 12, ldc=N + 8, key="gemm_f32 strided")
    ldc_odd = ((N + 3) // 4) * 4 + 5                      # ldc % 4 == 1: every row but the first starts off 16 B
    run_gemm(epi, M, N, K, lda=K + 4, ldw=K + 4, ldc=ldc_odd, key="gemm_f32 strided")
    run_gemm(epi, M, N, K, ldc=((N + 3) // 4) * 4 + 4, out_off=1, add_off=1, key="gemm_f32 strided")


@pytest.mark.parametrize("epi", EPIS)
def test_gemm_f32_no_bias_and_rowmask(epi):
    """bias = nullptr; rowmask rows come out zero for every epilogue but ADD2, which ignores the mask by design (gemm_f32.hip `masked`)"""
    for M, N, K in [(33, 65, 36), (1600, 1024, 100)]:
        run_gemm(epi, M, N, K, with_bias=False)
        mask = np.zeros(M, np.uint8)
        mask[::3] = 1
        mask[-1] = 1
        out = run_gemm(epi, M, N, K, rowmask=mask)
        if epi != F32_ADD2:
            assert (out[mask.astype(bool)] == 0).all()
        else:
            assert np.isfinite(out).all() and (out[:M][mask.astype(bool)] != 0).any()


@pytest.mark.parametrize("M,N,K", [(33, 65, 36), (1600, 1024, 100)])
def test_gemm_f32_res_scale_forms(M, N, K):
    """RES_SCALE with and without colscale (null => 1), with ldres != ldc"""
    run_gemm(F32_RES_SCALE, M, N, K, with_colscale=True, ldres=N + 12)
    run_gemm(F32_RES_SCALE, M, N, K, with_colscale=False, ldres=N + 5)


@pytest.mark.parametrize("M,N,K,rpc,nch", [(33, 65, 36, 4, 3), (200, 100, 132, 7, 4), (1600, 1024, 100, 64, 3)])
def test_gemm_f32_row_affine(M, N, K, rpc, nch):
    """ROWAFF_*: ch = (m / rows_per_ch) % nch wraps (M > rows_per_ch nch); null rowscale = identity; ROWAFF_RELU_RES in place (res == out)"""
    assert M > rpc * nch
    for epi in (F32_ROWAFF_RELU, F32_ROWAFF_RELU_RES):
        run_gemm(epi, M, N, K, rows_per_ch=rpc, nch=nch)
        run_gemm(epi, M, N, K, rows_per_ch=rpc, nch=nch, rowaff=False)
    run_gemm(F32_ROWAFF_RELU_RES, M, N, K, rows_per_ch=rpc, nch=nch, inplace_res=True)
    run_gemm(F32_ROWAFF_RELU_RES, M, N, K, rows_per_ch=rpc, nch=nch, ldres=N + 7)


@pytest.mark.parametrize("epi", [F32_BIAS, F32_SILU, F32_GELU])
@pytest.mark.parametrize("M,N,K", [(1, 1024, 256), (33, 65, 100), (200, 1026, 132)])
def test_gemm_f32_batched(epi, M, N, K):
    """nbatch = 22 (the AdaLN tables of a prepare()): distinct W and bias per z, out_bstride > M ldc with canaries between the slabs"""
    L, lib = _lib()
    nb, ldc = 22, N + 4
    bstride = (M + 2) * ldc + 3
    rng = np.random.default_rng(M + N + K + epi)
    A = f32(rng, M, K)
    Ws = [f32(rng, N, K, scale=1.0 / math.sqrt(K)) for _ in range(nb)]
    bs = [f32(rng, N) for _ in range(nb)]
    Ad = dev(A)
    Wd = [dev(w) for w in Ws]
    bd = [dev(b) for b in bs]
    Wv = torch.tensor([t.data_ptr() for t in Wd], dtype=torch.int64, device=DEV)
    bv = torch.tensor([t.data_ptr() for t in bd], dtype=torch.int64, device=DEV)
    outbuf = nan_buf(nb * bstride)
    a = L.GemmF32Args()
    a.A, a.lda, a.W, a.ldw, a.out, a.ldc, a.M, a.N, a.K = Ad.data_ptr(), K, Wd[0].data_ptr(), K, outbuf.data_ptr(), ldc, M, N, K
    a.nbatch, a.Wv, a.biasv, a.out_bstride = nb, Wv.data_ptr(), bv.data_ptr(), bstride
    L.check(lib.lemas_k_gemm_f32_ex(epi, C.byref(a), None), "gemm_f32_ex batched")
    flat = outbuf.cpu().numpy()
    A64 = A.astype(np.float64)
    for zi in range(nb):
        slab = flat[zi * bstride:(zi + 1) * bstride]
        o = slab[:M * ldc].reshape(M, ldc)
        assert np.isnan(o[:, N:]).all() and np.isnan(slab[M * ldc:]).all(), f"slab {zi}: wrote outside its M x N block"
        W64, b64 = Ws[zi].astype(np.float64), bs[zi].astype(np.float64)
        z = A64 @ W64.T + b64
        ref = act_ref(ACT[epi], z)
        bound = TOL.gemm_bound(TOL.gemm_acc_bound(A64, W64, b64, K), z, ref, ACT[epi])
        check(o[:, :N], ref, bound, f"batched slab {zi}", RATIOS, "gemm_f32 batched")


def test_gemm_f32_refusals():
    """K % 4, lda % 4, ldw % 4, M / N / K <= 0, nbatch without Wv / biasv: an error, and `out` untouched"""
    L, lib = _lib()
    A, W, b = torch.zeros(64 * 72, device=DEV), torch.zeros(64 * 72, device=DEV), torch.zeros(64, device=DEV)
    out = nan_buf(64 * 72)

    def args(**kw):
        a = L.GemmF32Args()
        a.A, a.lda, a.W, a.ldw, a.bias, a.out, a.ldc, a.M, a.N, a.K = A.data_ptr(), 64, W.data_ptr(), 64, b.data_ptr(), out.data_ptr(), 64, 16, 16, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    ok = args()
    assert lib.lemas_k_gemm_f32_ex(F32_BIAS, C.byref(ok), None) == 0
    out.fill_(float("nan"))
    bad = [dict(K=62), dict(K=30, lda=30, ldw=32), dict(lda=66), dict(ldw=62), dict(M=0), dict(N=0), dict(K=0), dict(M=-1),
           dict(nbatch=2), dict(nbatch=2, Wv=W.data_ptr())]
    for kw in bad:
        a = args(**kw)
        assert lib.lemas_k_gemm_f32_ex(F32_BIAS, C.byref(a), None) != 0, kw
    assert lib.lemas_k_gemm_f32_ex(9, C.byref(ok), None) != 0, "unknown epilogue"
    assert lib.lemas_k_gemm_f32_ex(-1, C.byref(ok), None) != 0, "unknown epilogue"
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused launch wrote"


# ---- gemv_f32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [F32_BIAS, F32_RELU, F32_SIGMOID])
@pytest.mark.parametrize("K", [4, 132, 1536, 3072])
def test_gemv_f32(epi, K):
    L, lib = _lib()
    for N in (1, 3, 4, 5, 1000):
        rng = np.random.default_rng(N * 10 + K + epi)
        ldw = K + 4
        a = f32(rng, K)
        Wm = np.full((N, ldw), np.nan, np.float32)
        Wm[:, :K] = f32(rng, N, K, scale=1.0 / math.sqrt(K))
        b = f32(rng, N)
        ad, Wd, bd = dev(a), dev(Wm), dev(b)
        out = nan_buf(N + 5)
        L.check(lib.lemas_k_gemv_f32(epi, ad.data_ptr(), Wd.data_ptr(), ldw, bd.data_ptr(), out.data_ptr(), N, K, None), "gemv_f32")
        o = out.cpu().numpy()
        assert np.isnan(o[N:]).all()
        A64, W64, b64 = a.astype(np.float64)[None], Wm[:, :K].astype(np.float64), b.astype(np.float64)
        z = A64 @ W64.T + b64
        ref = act_ref(ACT[epi], z)
        bound = TOL.gemm_bound(TOL.gemm_acc_bound(A64, W64, b64, K), z, ref, ACT[epi])
        check(o[None, :N], ref, bound, f"gemv N {N} K {K}", RATIOS, "gemv_f32")
        # the same row through the GEMM agrees within the sum of both bounds
        args = L.GemmF32Args()
        out2 = nan_buf(N)
        args.A, args.lda, args.W, args.ldw, args.bias, args.out, args.ldc, args.M, args.N, args.K = (
            ad.data_ptr(), K, Wd.data_ptr(), ldw, bd.data_ptr(), out2.data_ptr(), N, 1, N, K)
        L.check(lib.lemas_k_gemm_f32_ex(epi, C.byref(args), None), "gemm_f32 M = 1")
        g = out2.cpu().numpy()[None]
        check(g, o[None, :N], 2 * bound, f"gemv vs gemm N {N} K {K}")


def test_gemv_f32_refusals():
    L, lib = _lib()
    a, W, b = torch.zeros(1040, device=DEV), torch.zeros(64 * 1040, device=DEV), torch.zeros(64, device=DEV)
    out = nan_buf(64)
    p = lambda t, off=0: t.data_ptr() + 4 * off  # noqa: E731
    assert lib.lemas_k_gemv_f32(F32_BIAS, p(a), p(W), 1024, p(b), p(out), 64, 1024, None) == 0
    out.fill_(float("nan"))
    for epi, A_, W_, ldw, K in [(F32_BIAS, p(a, 1), p(W), 1024, 1024),       # A off 16 B
                                (F32_BIAS, p(a), p(W, 2), 1024, 1024),       # W off 16 B
                                (F32_BIAS, p(a), p(W), 1026, 1024),          # ldw % 4
                                (F32_BIAS, p(a), p(W), 1024, 1022),          # K % 4
                                (F32_BIAS, p(a), p(W), 1024, 0),
                                (F32_GELU, p(a), p(W), 1024, 1024), (F32_SILU, p(a), p(W), 1024, 1024),
                                (F32_RES_SCALE, p(a), p(W), 1024, 1024), (F32_ADD2, p(a), p(W), 1024, 1024),
                                (F32_ROWAFF_RELU, p(a), p(W), 1024, 1024)]:
        assert lib.lemas_k_gemv_f32(epi, A_, W_, ldw, p(b), p(out), 64, K, None) != 0, (epi, ldw, K)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- FFT ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = TOL.plan_lengths()


def test_fft_plan():
    """the plan's radices multiply to n for every accepted length; odd n, 7 2^k, n < 4 and n > 8192 are refused"""
    L, lib = _lib()
    assert len(LENGTHS) == 136 and LENGTHS[0] == 4 and LENGTHS[-1] == 8192 and 7680 in LENGTHS
    buf = (C.c_int32 * 14)()
    for n in LENGTHS:
        k = lib.lemas_k_fft_plan(n, buf, 14)
        assert k > 0, n
        rad = list(buf[:k])
        assert math.prod(rad) == n and set(rad) <= {2, 3, 4, 5}, (n, rad)
        assert rad == TOL.fft_radices(n), (n, rad)
    for n in [0, 1, 2, 3, 5, 9, 15, 45, 7, 14, 28, 56, 7 * 1024, 8194, 8200, 8640, 9000, 16384, -4]:
        assert lib.lemas_k_fft_plan(n, buf, 14) == -1, n
    accepted = set(LENGTHS)
    for n in range(4, 9000):
        ok = n in accepted
        assert (lib.lemas_k_fft_plan(n, buf, 14) > 0) == ok, n


def _fft_case(n, rows, ld, rng):
    L, lib = _lib()
    frames = f32(rng, rows, n)
    frames[rows // 2] *= 8.0                                 # rows of different scale in one launch
    spec = nan_buf(rows * ld + 7)
    fd = dev(frames)
    L.check(lib.lemas_k_rfft_rows(n, fd.data_ptr(), rows, spec.data_ptr(), ld, None), f"rfft n {n}")
    s = spec.cpu().numpy()
    assert np.isnan(s[rows * ld:]).all(), "rfft wrote past the last row"
    s = s[:rows * ld].reshape(rows, ld)
    nb = n // 2 + 1
    assert (s[:, 2 * nb:] == 0).all(), "the padding columns of a spectrum row are zero"
    ref = np.fft.rfft(frames.astype(np.float64), axis=1)
    bound = np.broadcast_to(TOL.fft_bound(n, TOL.pair_norms(frames))[:, None], (rows, nb))
    check(s[:, :nb], ref.real, bound, f"rfft re n {n} rows {rows}", RATIOS, "rfft_rows")
    check(s[:, nb:2 * nb], ref.imag, bound, f"rfft im n {n} rows {rows}", RATIOS, "rfft_rows")

    # inverse: a non-symmetric window, junk in the imaginary parts of DC and Nyquist (ignored, as irfft does)
    X = ref + (f32(rng, rows, nb) * 0.1 + 1j * f32(rng, rows, nb) * 0.1) * np.sqrt(n)
    X[:, 0] = X[:, 0].real + 1j * 1e3
    X[:, -1] = X[:, -1].real - 1j * 1e3
    Xs = np.full((rows, ld), np.nan, np.float32)
    Xs[:, :nb], Xs[:, nb:2 * nb] = X.real, X.imag
    Xs = Xs.astype(np.float32)
    window = (0.5 + np.arange(n) / n + 0.25 * np.sin(np.arange(n))).astype(np.float32)
    out = nan_buf(rows * n + 5)
    sd, wd = dev(Xs), dev(window)
    L.check(lib.lemas_k_irfft_rows(n, sd.data_ptr(), ld, rows, wd.data_ptr(), out.data_ptr(), None), f"irfft n {n}")
    o = out.cpu().numpy()
    assert np.isnan(o[rows * n:]).all(), "irfft wrote past the last row"
    Xr = Xs[:, :nb].astype(np.float64) + 1j * Xs[:, nb:2 * nb].astype(np.float64)
    Xr[:, 0] = Xr[:, 0].real
    Xr[:, -1] = Xr[:, -1].real
    time = np.fft.irfft(Xr, n, axis=1)
    ref_i = time * window.astype(np.float64)
    # the unnormalised inverse has the forward's per-sample bound on ||Z||_2 = sqrt(n) ||(a, b)||_2 of the time-domain pair, then w / n;
    # 1 / n, the window product and the final rounding add 3 u |out|
    bi = TOL.fft_bound(n, TOL.pair_norms(time) * math.sqrt(n))[:, None] * np.abs(window)[None, :] / n + 3 * U * np.abs(ref_i)
    check(o[:rows * n].reshape(rows, n), ref_i, bi, f"irfft n {n} rows {rows}", RATIOS, "irfft_rows")


@pytest.mark.parametrize("chunk", range(8))
def test_fft_every_length(chunk):
    """every plan length (136, every radix mix fft_plan_make builds) with rows 1 / 2 / 3 / 7 and ld = n + 2, n + 6 in turn"""
    for i, n in enumerate(LENGTHS[chunk::8]):
        rng = np.random.default_rng(n)
        rows = (1, 2, 3, 7)[i % 4]
        _fft_case(n, rows, n + 2 if i % 2 == 0 else n + 6, rng)


@pytest.mark.parametrize("n", [12, 30, 7680, 6144, 8192, 4374])
def test_fft_rows_and_ld(n):
    for rows in (1, 2, 3, 7):
        for ld in (n + 2, n + 6):
            _fft_case(n, rows, ld, np.random.default_rng(n + rows + ld))


def test_fft_refusals():
    L, lib = _lib()
    x, s = torch.zeros(4 * 64, device=DEV), nan_buf(4 * 70)
    for n, rows, ld in [(7, 1, 9), (14, 1, 16), (64, 0, 66), (64, 1, 65), (8194, 1, 8196)]:
        assert lib.lemas_k_rfft_rows(n, x.data_ptr(), rows, s.data_ptr(), ld, None) != 0, (n, rows, ld)
        assert lib.lemas_k_irfft_rows(n, s.data_ptr(), ld, rows, x.data_ptr(), x.data_ptr(), None) != 0, (n, rows, ld)
    torch.cuda.synchronize()
    assert torch.isnan(s).all()


# ---- res2net_step (prosody_oracle.tdnn: zero padding dil, ReLU, LayerNorm eps 1e-12) ----------------------------------------------
ECAPA_EPS = 1e-12


def _res2net_case(T, dil, with_add, ldx, ldadd, ldo, rng):
    L, lib = _lib()
    x = np.full((T, ldx), np.nan, np.float32)
    x[:, :64] = f32(rng, T, 64)
    add = None
    if with_add:
        add = np.full((T, ldadd), np.nan, np.float32)
        add[:, :64] = f32(rng, T, 64)
    W = f32(rng, 64, 64, 3, scale=1.0 / math.sqrt(192))
    b, lw, lb = f32(rng, 64, scale=0.1), (1.0 + 0.2 * f32(rng, 64)).astype(np.float32), f32(rng, 64, scale=0.1)
    xd, Wd, bd, lwd, lbd = dev(x), dev(W), dev(b), dev(lw), dev(lb)
    ad = dev(add) if with_add else None
    out = nan_buf(T * ldo + 9)
    L.check(lib.lemas_k_res2net_step(xd.data_ptr(), ldx, ad.data_ptr() if with_add else None, ldadd, T, dil, Wd.data_ptr(), bd.data_ptr(),
                                     lwd.data_ptr(), lbd.data_ptr(), ECAPA_EPS, out.data_ptr(), ldo, None), "res2net_step")
    o = out.cpu().numpy()
    assert np.isnan(o[T * ldo:]).all()
    o = o[:T * ldo].reshape(T, ldo)
    if ldo > 64:
        assert np.isnan(o[:, 64:]).all()
    xin = x[:, :64].astype(np.float64) + (add[:, :64].astype(np.float64) if with_add else 0.0)
    y, dy = TOL.conv_dil_ref(xin, W.astype(np.float64), b.astype(np.float64), dil)
    if with_add:                                   # x + add is rounded once more before the conv: u |x + add| per operand, one more u S
        dy = dy * (TOL.gemm_c(192) + 1) / TOL.gemm_c(192)
    yr = np.maximum(y, 0.0)
    t = torch.from_numpy(yr)
    ref = torch.nn.functional.layer_norm(t, (64,), torch.from_numpy(lw.astype(np.float64)), torch.from_numpy(lb.astype(np.float64)),
                                         eps=ECAPA_EPS).numpy()
    bound = TOL.ln_bound(yr, dy, lw.astype(np.float64), lb.astype(np.float64), ECAPA_EPS, ref)
    check(o[:, :64], ref, bound, f"res2net T {T} dil {dil} add {with_add}", RATIOS, "res2net_step")


@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 33, 130, 500])
def test_res2net_step(T):
    """dil 1 .. 16 (dil >= T included), add null and non-null, row pitches ldx / ldadd / ldo beyond 64"""
    for i, dil in enumerate([1, 2, 3, 5, 16]):
        rng = np.random.default_rng(T * 100 + dil)
        _res2net_case(T, dil, False, 64, 64, 64, rng)
        _res2net_case(T, dil, True, 68 + 4 * i, 72, 64 + 3 * i + 1, rng)


def test_res2net_step_refusals():
    L, lib = _lib()
    x, W = torch.zeros(64 * 80 + 64, device=DEV), torch.zeros(64 * 192 + 64, device=DEV)
    v = torch.zeros(128, device=DEV)
    out = nan_buf(64 * 80)
    p = lambda t, off=0: t.data_ptr() + 4 * off  # noqa: E731

    def call(x_=None, ldx=64, add=None, ldadd=64, T=16, dil=1, bias=None):
        return lib.lemas_k_res2net_step(x_ or p(x), ldx, add, ldadd, T, dil, p(W), bias or p(v), p(v), p(v), ECAPA_EPS, p(out), 64, None)
    assert call() == 0
    out.fill_(float("nan"))
    for kw in [dict(T=0), dict(T=-3), dict(dil=0), dict(dil=17), dict(ldx=66), dict(add=p(x), ldadd=66), dict(x_=p(x, 1)),
               dict(add=p(x, 2)), dict(bias=p(v, 1))]:
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- dwconv7_ln (lemas_oracle.OracleVocos: conv1d padding 3 per sample, groups = C, LayerNorm eps 1e-6) ---------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 7, 8, 939])
def test_dwconv7_ln(B, N):
    """with B > 1, sample b's window must not read sample b +- 1's frames: each sample sits on its own large constant"""
    L, lib = _lib()
    Cc = 512
    rng = np.random.default_rng(B * 1000 + N)
    x = f32(rng, B, N, Cc) + (np.arange(B, dtype=np.float32) * 100.0 - 100.0)[:, None, None] * (1.0 + np.arange(Cc) % 7)[None, None, :]
    x = x.astype(np.float32)
    w, b = f32(rng, Cc, 7, scale=0.3), f32(rng, Cc, scale=0.1)
    lw, lb = (1.0 + 0.2 * f32(rng, Cc)).astype(np.float32), f32(rng, Cc, scale=0.1)
    out = nan_buf(B * N * Cc + 11)
    xd, wd, bd, lwd, lbd = dev(x), dev(w), dev(b), dev(lw), dev(lb)
    L.check(lib.lemas_k_dwconv7_ln(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), lwd.data_ptr(), lbd.data_ptr(), out.data_ptr(), B, N, Cc, None),
            "dwconv7_ln")
    o = out.cpu().numpy()
    assert np.isnan(o[B * N * Cc:]).all()
    o = o[:B * N * Cc].reshape(B, N, Cc)
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    xp = np.zeros((B, N + 6, Cc))
    xp[:, 3:3 + N] = x64
    h = np.broadcast_to(b64, (B, N, Cc)).copy()
    S = np.broadcast_to(np.abs(b64), (B, N, Cc)).copy()
    for j in range(7):
        h += xp[:, j:j + N] * w64[:, j]
        S += np.abs(xp[:, j:j + N] * w64[:, j])
    dy = TOL.gemm_c(7) * U * S
    ref = torch.nn.functional.layer_norm(torch.from_numpy(h), (Cc,), torch.from_numpy(lw.astype(np.float64)),
                                         torch.from_numpy(lb.astype(np.float64)), eps=1e-6).numpy()
    bound = TOL.ln_bound(h, dy, lw.astype(np.float64), lb.astype(np.float64), 1e-6, ref)
    check(o, ref, bound, f"dwconv7_ln B {B} N {N}", RATIOS, "dwconv7_ln")


def test_dwconv7_ln_refuses_other_widths():
    L, lib = _lib()
    t = torch.zeros(8 * 1024, device=DEV)
    out = nan_buf(8 * 1024)
    for Cc in (256, 1024, 511):
        assert lib.lemas_k_dwconv7_ln(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), out.data_ptr(), 1, 4, Cc, None) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- col_stats / softmax_pool (prosody_oracle.asp: weights w, std = sqrt(clamp(sum w (x - mean)^2, eps)), eps 1e-12) ----------------
def _pool_inputs(T, Cc, rng, ldx):
    x = np.full((T, ldx), np.nan, np.float32)
    x[:, :Cc] = f32(rng, T, Cc)
    x[:, :Cc:4] = (1e3 + 0.01 * f32(rng, T, len(range(0, Cc, 4)))).astype(np.float32)     # large mean, small spread
    return x


@pytest.mark.parametrize("T", [1, 2, 3000])
def test_col_stats(T):
    L, lib = _lib()
    Cc, ldx = 100, 108
    x = _pool_inputs(T, Cc, np.random.default_rng(T), ldx)
    mean, std = nan_buf(Cc + 3), nan_buf(Cc + 3)
    xd = dev(x)
    L.check(lib.lemas_k_col_stats(xd.data_ptr(), ldx, T, Cc, ECAPA_EPS, mean.data_ptr(), std.data_ptr(), None), "col_stats")
    mo, so = mean.cpu().numpy(), std.cpu().numpy()
    assert np.isnan(mo[Cc:]).all() and np.isnan(so[Cc:]).all()
    x64 = x[:, :Cc].astype(np.float64)
    w = np.full((T, 1), 1.0 / T)
    m, var, dm, dvar = TOL.col_stats_bound(x64, w, T)
    check(mo[:Cc], m, dm, f"col_stats mean T {T}", RATIOS, "col_stats")
    check(so[:Cc], np.sqrt(np.maximum(var, ECAPA_EPS)), TOL.std_bound(var, dvar, ECAPA_EPS), f"col_stats std T {T}", RATIOS, "col_stats")


@pytest.mark.parametrize("T", [1, 2, 3000])
def test_softmax_pool(T):
    """softmax over time per column; one column is -1e4 everywhere but one frame (a one-hot attention)"""
    L, lib = _lib()
    Cc, ldx, lda = 100, 104, 112
    rng = np.random.default_rng(T + 5)
    x = _pool_inputs(T, Cc, rng, ldx)
    att = np.full((T, lda), np.nan, np.float32)
    att[:, :Cc] = f32(rng, T, Cc, scale=3.0)
    att[:, 7] = -1e4
    att[T // 2, 7] = 2.0
    mean, std = nan_buf(Cc + 3), nan_buf(Cc + 3)
    xd, ad = dev(x), dev(att)
    L.check(lib.lemas_k_softmax_pool(ad.data_ptr(), lda, xd.data_ptr(), ldx, T, Cc, ECAPA_EPS, mean.data_ptr(), std.data_ptr(), None), "softmax_pool")
    mo, so = mean.cpu().numpy(), std.cpu().numpy()
    assert np.isnan(mo[Cc:]).all() and np.isnan(so[Cc:]).all()
    a64, x64 = att[:, :Cc].astype(np.float64), x[:, :Cc].astype(np.float64)
    w = torch.softmax(torch.from_numpy(a64), 0).numpy()
    # relative error of each weight: the rounded argument a - max and the 1-ulp expf (frames whose weight underflows add nothing)
    eta = float(np.where(w > 1e-30, 4 * U + U * np.abs(a64 - a64.max(0)), 0.0).max())
    m, var, dm, dvar = TOL.col_stats_bound(x64, w, T, eta=eta)
    check(mo[:Cc], m, dm, f"softmax_pool mean T {T}", RATIOS, "softmax_pool")
    check(so[:Cc], np.sqrt(np.maximum(var, ECAPA_EPS)), TOL.std_bound(var, dvar, ECAPA_EPS), f"softmax_pool std T {T}", RATIOS, "softmax_pool")
    assert abs(mo[7] - x[T // 2, 7]) <= 2 * U * abs(x[T // 2, 7]) + 1e-30, "one-hot attention picks its frame"


# ---- ln_rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [4, 64, 1536, 4096])
@pytest.mark.parametrize("act_tanh", [0, 1])
def test_ln_rows(Cc, act_tanh):
    L, lib = _lib()
    T, ldx, ldo = 37, Cc + 8, Cc + 4
    rng = np.random.default_rng(Cc + act_tanh)
    x = np.full((T, ldx), np.nan, np.float32)
    x[:, :Cc] = f32(rng, T, Cc) + np.float32(3.0)
    w, b = (1.0 + 0.2 * f32(rng, Cc)).astype(np.float32), f32(rng, Cc, scale=0.1)
    for eps in (1e-12, 1e-5):
        out = nan_buf(T * ldo + 5)
        xd, wd, bd = dev(x), dev(w), dev(b)
        L.check(lib.lemas_k_ln_rows(xd.data_ptr(), ldx, T, Cc, wd.data_ptr(), bd.data_ptr(), eps, act_tanh, out.data_ptr(), ldo, None), "ln_rows")
        o = out.cpu().numpy()
        assert np.isnan(o[T * ldo:]).all()
        o = o[:T * ldo].reshape(T, ldo)
        assert np.isnan(o[:, Cc:]).all()
        x64 = x[:, :Cc].astype(np.float64)
        ref = torch.nn.functional.layer_norm(torch.from_numpy(x64), (Cc,), torch.from_numpy(w.astype(np.float64)),
                                             torch.from_numpy(b.astype(np.float64)), eps=eps).numpy()
        if act_tanh:
            ref = np.tanh(ref)
        bound = TOL.ln_bound(x64, np.zeros_like(x64), w.astype(np.float64), b.astype(np.float64), eps, ref, tanh=bool(act_tanh))
        check(o[:, :Cc], ref, bound, f"ln_rows C {Cc} tanh {act_tanh}", RATIOS, "ln_rows")


def test_ln_rows_refusals():
    L, lib = _lib()
    x, w = torch.zeros(8 * 4200, device=DEV), torch.zeros(4200, device=DEV)
    out = nan_buf(8 * 4200)
    p = lambda t, off=0: t.data_ptr() + 4 * off  # noqa: E731
    assert lib.lemas_k_ln_rows(p(x), 64, 4, 64, p(w), p(w), 1e-5, 0, p(out), 64, None) == 0
    out.fill_(float("nan"))
    for ldx, Cc, ldo, xo in [(66, 62, 64, 0), (66, 64, 64, 0), (64, 64, 66, 0), (4100, 4100, 4100, 0), (64, 64, 64, 1)]:
        assert lib.lemas_k_ln_rows(p(x, xo), ldx, 4, Cc, p(w), p(w), 1e-5, 0, p(out), ldo, None) != 0, (ldx, Cc, ldo, xo)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- mdx_groupnorm (GroupNorm(2, C) + ReLU, modes 0 / 1 / 2) ------------------------------------------------------------------------
def _gn_bound(x, mean, var, cols, gam, be, eps, pre, mode, other, ref):
    """per-lane fp32 chains of ceil(cols / 64) terms (sum and fmaf sum of squares), combined in double: the mean is off by
    gamma(k) E|x|, E[x^2] by gamma(k + 1) E[x^2]; var = E[x^2] - mean^2 (double) and rstd = 1 / sqrt(var + eps) rounded to fp32;
    out = relu((x - mean) rstd g + b) in fp32 (3 roundings), then * other or + other (1 more)"""
    k = math.ceil(cols / 64)
    dmean = TOL.gamma(k) * np.abs(x).mean() + 2 * U * abs(mean)
    dvar = TOL.gamma(k + 1) * (x ** 2).mean() + 2 * abs(mean) * dmean + dmean ** 2
    rstd = 1.0 / math.sqrt(var + eps)
    drstd = rstd * (dvar / (2 * (var + eps)) + U)
    d = np.abs(gam) * (dmean * rstd + np.abs(x - mean) * drstd) + 3 * U * (np.abs(pre) + np.abs(be))
    if mode == 1:
        d = d * np.abs(other) + U * np.abs(ref)
    elif mode == 2:
        d = d + U * np.abs(ref)
    return d


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_mdx_groupnorm(mode, B, offset):
    """(b, group) each with its own statistics; cols < ld; a large-mean input (what the double partial sums are for)"""
    L, lib = _lib()
    Cc, T, cols, ld = 6, 20, 37, 44
    rows = B * Cc * T
    rng = np.random.default_rng(mode * 10 + B + int(offset))
    x = np.full((rows, ld), np.nan, np.float32)
    base = f32(rng, rows, cols)
    # every (sample, group) on its own level and spread
    lvl = (np.arange(B * 2) * 5.0 - 3.0 + offset).repeat(Cc // 2 * T)[:, None]
    spr = (1.0 + np.arange(B * 2)).repeat(Cc // 2 * T)[:, None]
    x[:, :cols] = (base * spr + lvl).astype(np.float32)
    other = np.full((rows, ld), np.nan, np.float32)
    other[:, :cols] = f32(rng, rows, cols)
    g, be = (1.0 + 0.3 * f32(rng, Cc)).astype(np.float32), f32(rng, Cc, scale=0.2)
    eps = 1e-5
    out = nan_buf(rows * ld + 3)
    xd, od, gd, bd = dev(x), dev(other), dev(g), dev(be)
    L.check(lib.lemas_k_mdx_groupnorm(xd.data_ptr(), ld, cols, B, Cc, T, gd.data_ptr(), bd.data_ptr(), eps,
                                      od.data_ptr() if mode else None, mode, out.data_ptr(), None), "mdx_groupnorm")
    o = out.cpu().numpy()
    assert np.isnan(o[rows * ld:]).all()
    o = o[:rows * ld].reshape(rows, ld)
    assert np.isnan(o[:, cols:]).all(), "wrote past cols"
    x64 = x[:, :cols].astype(np.float64).reshape(B, Cc, T, cols)
    ref = np.empty_like(x64)
    bound = np.empty_like(x64)
    oth = other[:, :cols].astype(np.float64).reshape(B, Cc, T, cols)
    g64, b64 = g.astype(np.float64)[:, None, None], be.astype(np.float64)[:, None, None]
    for bi in range(B):
        for gi in range(2):
            sl = slice(gi * Cc // 2, (gi + 1) * Cc // 2)
            xs = x64[bi, sl]
            mean, var = xs.mean(), xs.var()
            pre = (xs - mean) / math.sqrt(var + eps) * g64[sl] + b64[sl]
            r = np.maximum(pre, 0.0)
            if mode == 1:
                r = r * oth[bi, sl]
            if mode == 2:
                r = r + oth[bi, sl]
            ref[bi, sl] = r
            bound[bi, sl] = _gn_bound(xs, mean, var, cols, g64[sl], b64[sl], eps, pre, mode, oth[bi, sl], r)
    check(o[:, :cols].reshape(B, Cc, T, cols), ref, bound, f"groupnorm mode {mode} B {B} offset {offset}", RATIOS,
          "mdx_groupnorm" + (" large mean" if offset else ""))


def test_mdx_groupnorm_refuses_odd_channels():
    L, lib = _lib()
    x = torch.zeros(5 * 4 * 8, device=DEV)
    out = nan_buf(5 * 4 * 8)
    assert lib.lemas_k_mdx_groupnorm(x.data_ptr(), 8, 8, 1, 5, 4, x.data_ptr(), x.data_ptr(), 1e-5, None, 0, out.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_zz_report():
    """the worst error / bound ratio per kernel of this run (pytest -s shows it): the headroom of each bound"""
    for k in sorted(RATIOS):
        print(f"f32-kernel-ratio {k}: {RATIOS[k]:.4f}")
