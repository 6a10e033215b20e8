"""Per-element error bounds of the exact-fp32 kernels against float64 references (tests/test_gpu_15_f32_kernels.py), and small float32
numpy models of the same algorithms (tests/test_f32_kernel_tolerance_cpu.py shows with them that every bound passes the correct
algorithm and rejects a plausible bug).

u = 2^-24 is the fp32 unit roundoff and gamma(n) = n u / (1 - n u) the classic bound of an n-term fp32 dot product or sum in any order
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1 / eq. 3.5): |fl(x . y) - x . y| <= gamma(n) |x| . |y|.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24


def gamma(n) -> np.ndarray | float:
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


# ---- exact-fp32 GEMM (csrc/gemm_f32.hip) ------------------------------------------------------------------------------------------
# The accumulator takes one rounded product-add per k (K of them, in a 16-k order of its own) and one more for the bias: K + 1 roundings.
# gamma(K + 1) <= (K + 2) u for every K here, so c = K + 2 bounds |acc + bias - (A . W^T + bias)| / (u (|A| |W|^T + |bias|)) for ANY
# summation order the kernel picks -- it does not depend on the 32-k tiling or on the MFMA's internal order.
def gemm_c(K: int) -> float:
    return K + 2.0


# Lipschitz constants of the epilogue activations: max |f'| (GELU-erf: x phi(x) + Phi(x) peaks at 1.1289; SiLU: 1.0998; sigmoid: 1/4)
LIP = {"bias": 1.0, "gelu": 1.129, "silu": 1.1, "relu": 1.0, "sigmoid": 0.25}


def gemm_acc_bound(A, W, bias, K: int) -> np.ndarray:
    """c u (|A| @ |W|^T + |bias|): the bound on the pre-activation z = A W^T + bias (A [M, K], W [N, K] float64 copies of the fp32 operands)"""
    S = np.abs(A) @ np.abs(W).T
    if bias is not None:
        S = S + np.abs(bias)[None, :]
    return gemm_c(K) * U * S


def act_eval_err(act: str, z: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """what evaluating the activation in fp32 adds on top of the final rounding u |ref|:
    gelu: 0.5 x (1 + erff(x / sqrt 2)) -- erff is good to 2 ulp of 1 (4 u), times 0.5 |x|: 2 u |z|, doubled;
    silu: x rcp(1 + exp2(-log2(e) x)) -- the exp2 argument's rounding is a relative error of u |x log2 e| in e^-x, exp2 and rcp 1 ulp each:
          (6 + 2 |z|) u |ref|;
    sigmoid: 1 / (1 + expf(-x)) with the 1-ulp expf, an add and a division: 6 u |ref|."""
    if act == "gelu":
        return 4.0 * U * np.abs(z)
    if act == "silu":
        return (6.0 + 2.0 * np.abs(z)) * U * np.abs(ref)
    if act == "sigmoid":
        return 6.0 * U * np.abs(ref)
    return np.zeros_like(ref)


def gemm_bound(acc_bound: np.ndarray, z: np.ndarray, ref: np.ndarray, act: str = "bias", scale=1.0, inner=None) -> np.ndarray:
    """|out - ref| <= |scale| Lip(act) c u (|A||W|^T + |bias|) + act_eval_err + u (|ref| + |inner|):
    scale = colscale (RES_SCALE) or the row-affine scale (ROWAFF_*), whose product / fma adds one rounding of the inner value `inner`;
    the final u |ref| is the rounding of the last add (residual, add operand) or of the activation's result."""
    b = np.abs(scale) * LIP[act] * acc_bound + act_eval_err(act, z, ref) + U * np.abs(ref)
    if inner is not None:
        b = b + U * np.abs(inner)
    return b


# ---- in-LDS real FFT (csrc/fft_kernels.hip) ---------------------------------------------------------------------------------------
# Per bin, the error of a Stockham FFT of the complex sequence z is a sum of independent rounding errors of every stage: each stage
# contributes about u ||z||_2 (its intermediates have norm sqrt(Ns) ||z||, and a bin sees n / Ns of them with unit weights), a radix-R
# butterfly performs at most ~R roundings per output, the twiddles themselves are rounded to fp32.  With log2(n) a bound on the number of
# butterfly levels weighted by their radix, c u log2(n) ||z||_2 per bin with c = 4 leaves room for the tail of the per-bin maximum over
# n bins (the float32 model in fft_model runs at 0.1 - 0.3 of it); a one-twiddle mistake is an O(|z|) error.  Two real rows share one
# complex transform (z = a + i b), so the norm is that of the PAIR.
FFT_C = 4.0


def fft_bound(n: int, pair_norm) -> np.ndarray | float:
    return FFT_C * U * math.log2(n) * np.asarray(pair_norm, dtype=np.float64)


def pair_norms(rows: np.ndarray) -> np.ndarray:
    """||z||_2 of the transform each row rides in: rows 2i and 2i + 1 share one (the last row of an odd count rides alone)"""
    sq = (rows.astype(np.float64) ** 2).sum(1)
    out = np.empty_like(sq)
    for r in range(0, len(sq), 2):
        s = sq[r] + (sq[r + 1] if r + 1 < len(sq) else 0.0)
        out[r] = s
        if r + 1 < len(sq):
            out[r + 1] = s
    return np.sqrt(out)


def fft_radices(n: int):
    """the plan fft_plan_make builds (the order of its stages), or None for a refused length"""
    if n < 4 or n & 1 or n > 8192:
        return None
    rad, m = [], n
    while m % 4 == 0:
        rad.append(4)
        m //= 4
    if m % 2 == 0:
        rad.append(2)
        m //= 2
    for r in (3, 5):
        while m % r == 0:
            rad.append(r)
            m //= r
    return rad if m == 1 else None


def plan_lengths():
    """every length fft_plan_make accepts: the even 2^a 3^b 5^c in [4, 8192]"""
    out = []
    for n in range(4, 8193, 2):
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1:
            out.append(n)
    return out


def fft_model(z: np.ndarray, radices, inverse: bool = False, conj_radix3_twiddle: bool = False) -> np.ndarray:
    """the kernel's Stockham transform in complex64 (twiddles computed in double, rounded to fp32), vectorised per stage.
    conj_radix3_twiddle: the bug of conjugating the first twiddle of every radix-3 butterfly."""
    n = len(z)
    t = np.arange(n)
    tw = np.exp(-2j * np.pi * t / n).astype(np.complex64)
    if inverse:
        tw = np.conj(tw)
    x = z.astype(np.complex64)
    Ns = 1
    for R in radices:
        M, step = n // R, n // (Ns * R)
        j = np.arange(M)
        q, k = j // Ns, j % Ns
        j0 = q * Ns * R + k
        v = []
        for r in range(R):
            w = tw[(r * k * step) % n]
            if conj_radix3_twiddle and R == 3 and r == 1:
                w = np.conj(w)
            v.append(x[j + r * M] * w)
        sgn = 1.0 if inverse else -1.0
        y = np.empty_like(x)
        for m in range(R):
            om = np.complex64(np.exp(sgn * 2j * np.pi * m / R))
            acc = v[0].copy()
            for r in range(1, R):
                acc = acc + v[r] * np.complex64(om ** r)
            y[j0 + m * Ns] = acc
        x = y
        Ns *= R
    return x


def rfft_rows_model(frames: np.ndarray, radices, **kw) -> np.ndarray:
    """rows -> the complex half spectra, two rows per complex transform, unpacked in float32 as rfft_rows_kernel does"""
    rows, n = frames.shape
    nb = n // 2 + 1
    out = np.zeros((rows, nb), np.complex128)
    for r in range(0, rows, 2):
        b = frames[r + 1] if r + 1 < rows else np.zeros(n, np.float32)
        Z = fft_model(frames[r].astype(np.complex64) + 1j * b.astype(np.complex64), radices, **kw)
        k = np.arange(nb)
        zk, zn = Z[k], Z[(n - k) % n]
        h = np.float32(0.5)
        out[r] = (h * (zk.real + zn.real)) + 1j * (h * (zk.imag - zn.imag))
        if r + 1 < rows:
            out[r + 1] = (h * (zk.imag + zn.imag)) + 1j * (-h * (zk.real - zn.real))
    return out


# ---- LayerNorm over a row of C values after an elementwise error dy (ln_rows, res2net_step, dwconv7_ln) --------------------------
# d LN / d y = rstd diag(w) (I - 1 1^T / C - yhat yhat^T / C): every row of the projection has 2-norm <= 1, so an input error dy moves
# out_c by at most |w_c| rstd ||dy||_2.  The statistics' own rounding: the mean of C values is off by gamma(C + 1) mean|y| (a shift of
# yhat by rstd times that), the variance and rstd relatively by gamma(C + 4) (sum of squares, division, sqrt, reciprocal): yhat moves by
# |yhat| gamma(C + 4); the affine adds u (|out| + |b|) and a tanh after it at most 4 u |out| more.
def ln_bound(y: np.ndarray, dy: np.ndarray, w: np.ndarray, b: np.ndarray, eps: float, out_ref: np.ndarray, tanh: bool = False) -> np.ndarray:
    C = y.shape[-1]
    mean = y.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((y - mean) ** 2).mean(-1, keepdims=True) + eps)
    yhat = (y - mean) * rstd
    dnorm = np.sqrt((dy ** 2).sum(-1, keepdims=True))
    t = np.abs(w) * (rstd * (dnorm + gamma(C + 1) * np.abs(y).mean(-1, keepdims=True)) + np.abs(yhat) * gamma(C + 4))
    pre = yhat * w + b
    t = t + U * (np.abs(pre) + np.abs(b)) * 2.0
    if tanh:
        t = t + 4.0 * U * np.abs(out_ref)        # tanh is 1-Lipschitz: the pre-activation bound carries through
    return t


def res2net_model(x: np.ndarray, W: np.ndarray, bias, lnw, lnb, eps: float, dil: int) -> np.ndarray:
    """float32 model of res2net_step: time-major x [T][64], W [64][64][3], zero padding dil"""
    T = x.shape[0]
    xp = np.zeros((T + 2 * dil, 64), np.float32)
    xp[dil:dil + T] = x
    acc = np.zeros((T, 64), np.float32)
    for j in range(3):
        acc += xp[j * dil:j * dil + T] @ W[:, :, j].T.astype(np.float32)
    y = np.maximum(acc + bias.astype(np.float32), np.float32(0))
    m = y.mean(-1, keepdims=True, dtype=np.float32)
    v = ((y - m) ** 2).mean(-1, keepdims=True, dtype=np.float32)
    return (y - m) / np.sqrt(v + np.float32(eps)) * lnw + lnb


def conv_dil_ref(x: np.ndarray, W: np.ndarray, bias, dil: int) -> tuple[np.ndarray, np.ndarray]:
    """float64 conv1d (3 taps, zero padding dil, time-major) and the gemm_acc_bound of each output (K = 192 terms + bias)"""
    T = x.shape[0]
    xp = np.zeros((T + 2 * dil, x.shape[1]))
    xp[dil:dil + T] = x
    y = np.zeros((T, W.shape[0]))
    S = np.zeros_like(y)
    for j in range(3):
        y += xp[j * dil:j * dil + T] @ W[:, :, j].T
        S += np.abs(xp[j * dil:j * dil + T]) @ np.abs(W[:, :, j]).T
    y += bias
    S += np.abs(bias)
    return y, gemm_c(3 * x.shape[1]) * U * S


# ---- weighted column statistics (col_stats: uniform weights; softmax_pool: softmax weights) --------------------------------------
# The kernels sum a column in 64 strided per-thread chains of ceil(T / 64) terms and then a 6-level tree: gamma(ceil(T / 64) + 7) per sum
# (the division included).  Softmax weights e_t = exp(a_t - max) carry a relative error eta_t <= 4 u + u |a_t - max| (the rounded argument
# and the 1-ulp expf).  mean = sum e x / sum e: |dm| <= (g + eta) (sum w |x| + |m|) + u |m|.  var = sum e (x - m)^2 / sum e with the
# computed m: |dvar| <= (g + eta) 2 var + 2 |dm| sum w |x - m|... + dm^2, std = sqrt(max(var, eps)): |dstd| <= |dvar| / (2 std) + u std.
def col_stats_bound(x: np.ndarray, w: np.ndarray, T: int, eta: np.ndarray | float = 0.0):
    g = gamma(math.ceil(T / 64) + 7)
    eta_max = np.max(eta) if np.ndim(eta) else eta
    m = (w * x).sum(0)
    dm = (g + eta_max) * ((w * np.abs(x)).sum(0) + np.abs(m)) + U * np.abs(m)
    var = (w * (x - m) ** 2).sum(0)
    dvar = (g + eta_max) * 2.0 * var + 2.0 * dm * (w * np.abs(x - m)).sum(0) + dm ** 2
    return m, var, dm, dvar


def std_bound(var: np.ndarray, dvar: np.ndarray, eps: float) -> np.ndarray:
    std = np.sqrt(np.maximum(var, eps))
    return dvar / (2.0 * std) + 2.0 * U * std


def check(out, ref, bound, what: str = "", ratios: dict | None = None, key: str | None = None) -> float:
    """assert |out - ref| <= bound element by element (NaN in out fails); returns the worst error / bound ratio, recorded in ratios[key]"""
    out, ref, bound = (np.asarray(a, dtype=np.float64) for a in (out, ref, bound))
    err = np.abs(out - ref)
    bad = ~(err <= bound)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    if ratios is not None and key is not None:
        ratios[key] = max(ratios.get(key, 0.0), ratio)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), -1)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} elements outside the bound; worst at {i}: out {out[i]!r} ref {ref[i]!r} "
                             f"err {err[i]:.3e} bound {bound[i]:.3e}")
    return ratio
