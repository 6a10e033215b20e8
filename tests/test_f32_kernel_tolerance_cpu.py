"""CPU tier: the per-element bounds of tests/test_gpu_15_f32_kernels.py are tight enough to matter.  For each bound, a float32 model of
the CORRECT algorithm stays inside it, and a model with one plausible bug, at the shapes the GPU test uses, falls outside it."""
import math

import numpy as np
import pytest

import f32_tolerance as TOL


def _f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _gemm_case(M, N, K, seed=0):
    rng = np.random.default_rng(seed)
    A, W, b = _f32(rng, M, K), _f32(rng, N, K, scale=1.0 / math.sqrt(K)), _f32(rng, N)
    A64, W64, b64 = A.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    z = A64 @ W64.T + b64
    return A, W, b, z, TOL.gemm_acc_bound(A64, W64, b64, K)


def _violates(out, ref, bound):
    return bool((np.abs(np.asarray(out, np.float64) - ref) > bound).any())


@pytest.mark.parametrize("M,N,K", [(33, 65, 36), (65, 100, 132), (31, 1026, 1024), (1600, 64, 100)])
def test_gemm_bound_passes_fp32_and_catches_a_dropped_k_tile(M, N, K):
    A, W, b, z, accb = _gemm_case(M, N, K)
    good = (A @ W.T + b).astype(np.float32)
    TOL.check(good, z, TOL.gemm_bound(accb, z, z))
    Ad = A.copy()
    Ad[:, 32:64] = 0.0                                  # one K-tile of 32 never accumulated
    assert _violates((Ad @ W.T + b), z, TOL.gemm_bound(accb, z, z))


@pytest.mark.parametrize("M,N,K", [(1, 3, 4), (33, 65, 36), (65, 1026, 1024)])
def test_gemm_bound_catches_bias_off_by_one_column(M, N, K):
    A, W, b, z, accb = _gemm_case(M, N, K, seed=1)
    bad = A @ W.T + np.roll(b, -1)                      # column n gets bias[n + 1]
    assert _violates(bad, z, TOL.gemm_bound(accb, z, z))


@pytest.mark.parametrize("M,N,K,rpc,nch", [(33, 65, 36, 4, 3), (200, 100, 132, 7, 4)])
def test_row_affine_bound_catches_the_neighbouring_channel(M, N, K, rpc, nch):
    A, W, b, z, accb = _gemm_case(M, N, K, seed=2)
    rng = np.random.default_rng(3)
    rs = (rng.uniform(0.25, 2.0, nch) * rng.choice([-1.0, 1.0], nch)).astype(np.float32)
    rh = _f32(rng, nch)
    ch = (np.arange(M) // rpc) % nch
    inner = rs[ch][:, None] * z + rh[ch][:, None]
    ref = np.maximum(inner, 0.0)
    bound = TOL.gemm_bound(accb, z, ref, "relu", scale=rs[ch][:, None], inner=inner)
    zf = (A @ W.T + b).astype(np.float32)
    TOL.check(np.maximum(rs[ch][:, None] * zf + rh[ch][:, None], 0), ref, bound)
    chb = ch.copy()
    chb[rpc] = (ch[rpc] + 1) % nch                      # one row takes the next channel's scale / shift
    assert _violates(np.maximum(rs[chb][:, None] * zf + rh[chb][:, None], 0), ref, bound)


@pytest.mark.parametrize("M,N,K", [(33, 65, 36), (1600, 64, 100)])
def test_res_scale_bound_catches_an_ignored_colscale(M, N, K):
    A, W, b, z, accb = _gemm_case(M, N, K, seed=4)
    rng = np.random.default_rng(5)
    res = _f32(rng, M, N)
    cs = (rng.uniform(0.25, 2.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    ref = res + cs * z
    bound = TOL.gemm_bound(accb, z, ref, scale=cs[None, :], inner=cs * z)
    zf = (A @ W.T + b).astype(np.float32)
    TOL.check(res + cs * zf, ref, bound)
    assert _violates(res + zf, ref, bound)


@pytest.mark.parametrize("n", [12, 30, 90, 7680, 4374])
def test_fft_bound_passes_the_model_and_catches_a_conjugated_radix3_twiddle(n):
    rad = TOL.fft_radices(n)
    assert 3 in rad and rad.index(3) > 0                # a radix-3 stage with k > 0 twiddles
    rng = np.random.default_rng(n)
    x = _f32(rng, 3, n)
    ref = np.fft.rfft(x.astype(np.float64), axis=1)
    bound = TOL.fft_bound(n, TOL.pair_norms(x))[:, None]
    TOL.check(np.abs(TOL.rfft_rows_model(x, rad) - ref), 0.0, bound)
    assert _violates(np.abs(TOL.rfft_rows_model(x, rad, conj_radix3_twiddle=True) - ref), 0.0, bound)


def test_plan_lengths_and_radices():
    L = TOL.plan_lengths()
    assert len(L) == 136 and all(math.prod(TOL.fft_radices(n)) == n for n in L)
    assert TOL.fft_radices(7680) == [4, 4, 4, 4, 2, 3, 5] and TOL.fft_radices(14) is None and TOL.fft_radices(8194) is None


@pytest.mark.parametrize("T,dil", [(17, 2), (130, 5), (500, 16), (33, 3)])
def test_res2net_bound_catches_a_dilation_off_by_one(T, dil):
    rng = np.random.default_rng(T + dil)
    x = _f32(rng, T, 64)
    W = _f32(rng, 64, 64, 3, scale=1.0 / math.sqrt(192))
    b, lw, lb = _f32(rng, 64, scale=0.1), (1.0 + 0.2 * _f32(rng, 64)).astype(np.float32), _f32(rng, 64, scale=0.1)
    y, dy = TOL.conv_dil_ref(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64), dil)
    yr = np.maximum(y, 0.0)
    m = yr.mean(-1, keepdims=True)
    ref = (yr - m) / np.sqrt(((yr - m) ** 2).mean(-1, keepdims=True) + 1e-12) * lw + lb
    bound = TOL.ln_bound(yr, dy, lw.astype(np.float64), lb.astype(np.float64), 1e-12, ref)
    TOL.check(TOL.res2net_model(x, W, b, lw, lb, 1e-12, dil), ref, bound)
    assert _violates(TOL.res2net_model(x, W, b, lw, lb, 1e-12, dil - 1 if dil > 1 else 2), ref, bound)
