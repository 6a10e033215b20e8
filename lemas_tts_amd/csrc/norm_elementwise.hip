// HBM-bound row/elementwise kernels of the DiT step loop and its per-utterance setup (gfx950).
//   ln_mod        modules.py:314,637 / :335  LayerNorm(no affine, eps 1e-6) * (1 + scale) + shift  -> bf16
//   cfg_euler     cfm.py:420-424 + the Euler update of torchdiffeq (call site cfm.py:456)
//   ode_stage     the same CFG + clamp, then one stage of torchdiffeq's fixed-grid midpoint / rk4 (option "ode_method")
//   rope_table    x_transformers RotaryEmbedding.forward_from_seq_len (call site dit.py:236)
//   misc          fp32->bf16 conversion / weight re-layout used when weights are loaded
#include "common.h"
#include "kernels.h"
#include "ln_core.h"

namespace {

// one wave per ROWS rows; D = 1024 -> 16 elements per lane and row as 2 groups of 8 consecutive columns (2 x float4 loads each), so the
// bf16 result leaves as 16-B write-through (sc1) stores: the next kernel (a GEMM on other XCDs) reads it from memory anyway and
// the launch does not end on an L2 write-back of 3.9 MB.  The row arithmetic is ln_core.h's (shared with the GEMM's LN tail).
template <int D, int ROWS>
__global__ __launch_bounds__(256) void ln_mod_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int M,
                                                     const float* __restrict__ tab, int tab_stride, int scale_off,
                                                     int shift_off, const int* __restrict__ step_idx,
                                                     const int* __restrict__ live_len, int pitch, int batch) {
  static_assert(D == LN_D, "row width");
  static_assert(128 % ROWS == 0, "a wave's rows share one 128-row block");
  constexpr int PER = LN_PER;
  // every kernel argument in ONE scalar request: left alone the compiler fetched them where they are first used -- M, then live_len, then the
  // pointers, then step_idx[0], four dependent scalar-memory round trips (~0.2 us each) in front of the first row load of a ~5 us kernel
  // (not step_idx, which is read with a scalar load: handing a pointer to an asm statement makes it "captured" and its loads vector loads)
  asm volatile("" ::"s"(x), "s"(out), "s"(M), "s"(tab), "s"(tab_stride), "s"(scale_off), "s"(shift_off), "s"(live_len), "s"(pitch), "s"(batch));
  // the step index: REQUESTED here, in the entry block (a scalar load there; behind the row tests the compiler made it a vector load with a
  // vmcnt(0) of its own), and looked at only after the row loads below are out
  int st = 0;
  if (step_idx) st = step_idx[0];
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
  if (row0 >= M) return;
  if (live_len && row_block_dead(live_len, row0 & ~127, pitch, batch)) return;     // ragged batch: the block lies in a sample's padding
  const int lane = threadIdx.x & 63;
  // ROWS rows per wave: all their loads are issued before the first reduction (a wave with one row has 64 B per lane in flight
  // and then sits through two dependent shuffle reductions; the kernel is latency-, not bandwidth-bound at batch 1)
  float4 v[ROWS][PER][2];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int row = row0 + r < M ? row0 + r : M - 1;
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * D);
#pragma unroll
    for (int i = 0; i < PER; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) v[r][i][h] = xr[(lane + 64 * i) * 2 + h];
  }
  // the row loads are on their way BEFORE the step index is looked at (the modulation vectors' addresses need it)
  __builtin_amdgcn_sched_barrier(0);
  const float* base = tab + (size_t)st * tab_stride;
  float4 a[PER][2], b[PER][2];
  ln_load_vec(base + scale_off, lane, a);
  ln_load_vec(base + shift_off, lane, b);
  // ... and the modulation vectors are requested HERE, behind the rows and ahead of any arithmetic: left alone the compiler sinks each of
  // these (L2-resident) loads to its first use, and the row's store waits through three more memory round trips one after the other
#pragma unroll
  for (int i = 0; i < PER; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) { asm volatile("" : "+v"(a[i][h].x)); asm volatile("" : "+v"(b[i][h].x)); }
  // (the rows pass through the same gate: without it the first partial sums are scheduled ahead of the vector requests)
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int i = 0; i < PER; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(v[r][i][h].x), "+v"(v[r][i][h].y), "+v"(v[r][i][h].z), "+v"(v[r][i][h].w));
#pragma unroll
  for (int r = 0; r < ROWS; ++r) ln_row_store(v[r], a, b, out + (size_t)(row0 + r) * D, lane, row0 + r < M);
}

// ln fold (GemmParams): the entry of a lane's block chain, where no gate + residual GEMM precedes the first LayerNorm.  Writes what
// such a GEMM's epilogue would: xs = bf16(x (1 + scale)) and the (sum, sum of squares) pair of each 32-column slot of each row, added
// up in the same order (4-column groups, then a binary tree over the slot's 8 groups).
// Row image as in ln_core.h: v[i][h] = row[8 (lane + 64 i) + 4 h ..], so slot (lane >> 2) + 16 i is shared by 4 consecutive lanes.
template <int ROWS>
__global__ __launch_bounds__(256) void ln_prep_kernel(const float* __restrict__ x, bf16_t* __restrict__ xs, float* __restrict__ part, int M,
                                                      const float* __restrict__ tab, int tab_stride, int scale_off,
                                                      const int* __restrict__ step_idx) {
  constexpr int PER = LN_PER, D = LN_D;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
  if (row0 >= M) return;
  const int lane = threadIdx.x & 63;
  const float* base = tab + (step_idx ? (size_t)step_idx[0] * tab_stride : 0);
  float4 v[ROWS][PER][2];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int row = row0 + r < M ? row0 + r : M - 1;
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * D);
#pragma unroll
    for (int i = 0; i < PER; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) v[r][i][h] = xr[(lane + 64 * i) * 2 + h];
  }
  float4 a[PER][2];
  ln_load_vec(base + scale_off, lane, a);
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int row = row0 + r;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      float g1[2], g2[2];
      bf16x8 o;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 t = v[r][i][h];
        g1[h] = (t.x + t.y) + (t.z + t.w);
        g2[h] = __builtin_fmaf(t.x, t.x, __builtin_fmaf(t.y, t.y, __builtin_fmaf(t.z, t.z, t.w * t.w)));
        o[4 * h + 0] = (bf16_t)(t.x * (1.0f + a[i][h].x)); o[4 * h + 1] = (bf16_t)(t.y * (1.0f + a[i][h].y));
        o[4 * h + 2] = (bf16_t)(t.z * (1.0f + a[i][h].z)); o[4 * h + 3] = (bf16_t)(t.w * (1.0f + a[i][h].w));
      }
      float s1 = g1[0] + g1[1], s2 = g2[0] + g2[1];
#pragma unroll
      for (int m = 1; m < 4; m <<= 1) { s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64); }
      if (row < M) {
        store_wt_b128(xs + (size_t)row * D + (lane + 64 * i) * 8, __builtin_bit_cast(u32x4, o));
        if ((lane & 3) == 0) *reinterpret_cast<float2*>(part + ((size_t)row * (D / 32) + (lane >> 2) + 16 * i) * 2) = make_float2(s1, s2);
      }
    }
  }
}

// ln-fold tables, once per t-grid (prepare()): for every site (a LayerNorm + the GEMM behind it) and ODE step
//   c1[n] = sum_k (1 + scale_k) W[n][k],   c2[n] = sum_k shift_k W[n][k] + bias[n].
// The sums run on the bf16 MFMA GEMM against the SAME bf16 weights the step loop multiplies with: (1 + scale) and shift are cut into two
// bf16 terms each (hi = bf16(v), lo = bf16(v - hi): 16 mantissa bits, products exact in the fp32 accumulator), stacked as the rows
// [hi(1+scale) | lo | hi(shift) | lo] x S of one small A matrix per site, and the four partial rows are added up afterwards.
__global__ __launch_bounds__(256) void ln_fold_split_kernel(const float* __restrict__ tab, int tab_stride, int S, int d,
                                                            const LnFoldSite* __restrict__ sites, bf16_t* __restrict__ A) {
  const int step = blockIdx.x, site = blockIdx.y;
  const LnFoldSite st = sites[site];
  const float* row = tab + (size_t)step * tab_stride;
  bf16_t* a = A + (size_t)site * 4 * S * d;
  for (int k = threadIdx.x; k < d; k += 256) {
    const float sc = 1.0f + row[st.scale_off + k], sh = row[st.shift_off + k];
    const bf16_t sch = (bf16_t)sc, shh = (bf16_t)sh;
    a[(size_t)(0 * S + step) * d + k] = sch;
    a[(size_t)(1 * S + step) * d + k] = (bf16_t)(sc - (float)sch);
    a[(size_t)(2 * S + step) * d + k] = shh;
    a[(size_t)(3 * S + step) * d + k] = (bf16_t)(sh - (float)shh);
  }
}
__global__ __launch_bounds__(256) void ln_fold_combine_kernel(const LnFoldSite* __restrict__ sites, int S, float* __restrict__ tab, int tab_stride) {
  const LnFoldSite st = sites[blockIdx.z];
  const int step = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= st.N) return;
  const float* t = st.tmp;
  const size_t N = (size_t)st.N;
  float* row = tab + (size_t)step * tab_stride;
  row[st.c1_off + n] = t[(size_t)(0 * S + step) * N + n] + t[(size_t)(1 * S + step) * N + n];
  row[st.c2_off + n] = (t[(size_t)(2 * S + step) * N + n] + t[(size_t)(3 * S + step) * N + n]) + st.bias[n];
}

// Same row pass, written as MXFP8 for the fp8 GEMMs: e4m3 bytes + one E8M0 scale per 32 columns.  A 32-column block is
// the float4s of 8 consecutive lanes (for each of the PER strides), so the block max is three xor-shuffles.
template <int D>
__global__ __launch_bounds__(256) void ln_mod_f8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out8,
                                                        uint8_t* __restrict__ mx, int M, const float* __restrict__ tab,
                                                        int tab_stride, int scale_off, int shift_off,
                                                        const int* __restrict__ step_idx) {
  constexpr int PER = D / 256;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float* base = tab + (step_idx ? (size_t)step_idx[0] * tab_stride : 0);
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * D);
  float4 v[PER];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    v[i] = xr[lane + 64 * i];
    s += v[i].x + v[i].y + v[i].z + v[i].w;
  }
  const float mean = wave_sum(s) * (1.0f / D);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
    q += a * a + b * b + c * c + d * d;
  }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + 1e-6f);
  const float4* sc = reinterpret_cast<const float4*>(base + scale_off);
  const float4* sh = reinterpret_cast<const float4*>(base + shift_off);
  unsigned int* orow = reinterpret_cast<unsigned int*>(out8 + (size_t)row * D);
  uint8_t* mrow = mx + (size_t)row * (D / 32);
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const float4 a = sc[lane + 64 * i], b = sh[lane + 64 * i];
    const float o0 = (v[i].x - mean) * rstd * (1.0f + a.x) + b.x, o1 = (v[i].y - mean) * rstd * (1.0f + a.y) + b.y;
    const float o2 = (v[i].z - mean) * rstd * (1.0f + a.z) + b.z, o3 = (v[i].w - mean) * rstd * (1.0f + a.w) + b.w;
    float amax = fmaxf(fmaxf(fabsf(o0), fabsf(o1)), fmaxf(fabsf(o2), fabsf(o3)));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
    const int e = mx_exponent(amax);
    const float inv = mx_inv_scale(e);
    orow[lane + 64 * i] = pack_fp8x4(o0 * inv, o1 * inv, o2 * inv, o3 * inv);
    if ((lane & 7) == 0) mrow[(lane >> 3) + 8 * i] = (uint8_t)(e + 127);
  }
}

// fp32 rows -> MXFP8: one thread per 32-column block
__global__ __launch_bounds__(256) void mx_quant_rows_kernel(const float* __restrict__ x, int M, int K, uint8_t* __restrict__ out8,
                                                            uint8_t* __restrict__ mx) {
  const int nb = K >> 5;
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (t >= (size_t)M * nb) return;
  const float4* src = reinterpret_cast<const float4*>(x + t * 32);
  float4 v[8];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = src[i];
    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v[i].x), fabsf(v[i].y))), fmaxf(fabsf(v[i].z), fabsf(v[i].w)));
  }
  const int e = mx_exponent(amax);
  const float inv = mx_inv_scale(e);
  unsigned int* dst = reinterpret_cast<unsigned int*>(out8 + t * 32);
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = pack_fp8x4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
  mx[t] = (uint8_t)(e + 127);
}

// weights [N][K] -> e4m3 with a per-row fp32 scale: one wave per row
__global__ __launch_bounds__(256) void w_quant_f8_kernel(const float* __restrict__ w, int N, int K, uint8_t* __restrict__ out8,
                                                         float* __restrict__ scale) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const float4* src = reinterpret_cast<const float4*>(w + (size_t)row * K);
  float amax = 0.f;
  for (int c = lane; c < K / 4; c += 64) {
    const float4 v = src[c];
    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  amax = wave_max(amax);
  const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
  unsigned int* dst = reinterpret_cast<unsigned int*>(out8 + (size_t)row * K);
  for (int c = lane; c < K / 4; c += 64) {
    const float4 v = src[c];
    dst[c] = pack_fp8x4(v.x / sc, v.y / sc, v.z / sc, v.w / sc);
  }
  if (lane == 0) scale[row] = sc;
}

// e4m3 weights [N][K] with a per-row fp32 scale -> bf16 (the value the fp8 MFMA would see, in the bf16 kernels' operand format)
__global__ __launch_bounds__(256) void f8_to_bf16_kernel(const uint8_t* __restrict__ w8, const float* __restrict__ scale, int N, int K,
                                                         bf16_t* __restrict__ out) {
  const size_t total = (size_t)N * (K / 4);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / (K / 4));
    const int packed = reinterpret_cast<const int*>(w8)[i];
    const float sc = scale[row];
    bf16x4 o;
    o[0] = (bf16_t)(__builtin_amdgcn_cvt_f32_fp8(packed, 0) * sc);
    o[1] = (bf16_t)(__builtin_amdgcn_cvt_f32_fp8(packed, 1) * sc);
    o[2] = (bf16_t)(__builtin_amdgcn_cvt_f32_fp8(packed, 2) * sc);
    o[3] = (bf16_t)(__builtin_amdgcn_cvt_f32_fp8(packed, 3) * sc);
    reinterpret_cast<bf16x4*>(out)[i] = o;
  }
}

__global__ __launch_bounds__(256) void cfg_euler_kernel(float* __restrict__ y, const float* __restrict__ pred, int rows,
                                                        int cols, const float* __restrict__ dt_tab,
                                                        const float* __restrict__ cfg_tab, int* step_idx,
                                                        float* __restrict__ traj, int use_cfg) {
  const int k = step_idx[0];
  const float dt = dt_tab[k], cg = cfg_tab[k];
  const size_t total = (size_t)rows * cols;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float pc = pred[i];
    float f = pc;
    if (use_cfg) {
      const float pu = pred[total + i];
      f = pc + (pc - pu) * cg;
      f = fminf(fmaxf(f, -20.0f), 20.0f);
    }
    const float yn = y[i] + dt * f;
    y[i] = yn;
    if (traj) traj[(size_t)(k + 1) * total + i] = yn;
  }
}

// one STAGE of a higher-order fixed-grid solver (torchdiffeq 0.2.4 fixed_grid.Midpoint / rk_common.rk4_alt_step_func, dt = t1 - t0,
// y1 = y0 + dy), with the CFG + clamp of cfm.py:420-424 at the stage's own time (cfg_tab is per EVALUATION).  The evaluation counter
// selects the stage's row of `stages`: its kind and dt.  Buffers: base = y0 of the step, k1..k3 = the rk4 slopes; y = the next stage's
// input, or y1 at the step's last stage.  Products and sums are rounded one by one in torch's order (no FMA contraction), so the
// solve equals the same solver composed on the host from single forwards (tests/test_gpu_16_ode_methods.py):
//   MID0   f0 = f(t0, y0):               base = y0;  y = y0 + f0 * half_dt          (c = half_dt = 0.5 * dt)
//   MID1   f1 = f(t0 + half_dt, y_mid):  y = y0 + dt * f1
//   RK0    k1 = f(t0, y0):               base = y0;  k1;  y = y0 + dt * k1 * (1/3)
//   RK1    k2 = f(t0 + dt/3, .):         k2;  y = y0 + dt * (k2 - k1 * (1/3))
//   RK2    k3 = f(t0 + 2 dt/3, .):       k3;  y = y0 + dt * (k1 - k2 + k3)
//   RK3    k4 = f(t1, .):                y = y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
// A product that no FMA can absorb: HIP's __fmul_rn is a plain `*`, and under this build's -O3 contraction (which ignores
// `#pragma clang fp contract`) `a * b + c` becomes one v_fma -- one ulp of difference in a stage input then flips bf16 roundings of
// the next network evaluation.  The empty asm makes the rounded product opaque to the combiner; the add after it stays an add.
__device__ __forceinline__ float mul_rn(float a, float b) {
  float p = a * b;
  __asm__ volatile("" : "+v"(p));
  return p;
}

__device__ __forceinline__ float ode_cfg(float pc, float pu, float cg) {
  return fminf(fmaxf(pc + mul_rn(pc - pu, cg), -20.0f), 20.0f);
}

__device__ __forceinline__ float ode_stage_elem(int kind, float dt, float c, float f, float y0, float a1, float a2, float a3) {
  const float third = 1.0f / 3.0f;
  switch (kind) {
    case ODE_MID0: return y0 + mul_rn(f, c);
    case ODE_MID1: return y0 + mul_rn(dt, f);
    case ODE_RK0: return y0 + mul_rn(mul_rn(dt, f), third);
    case ODE_RK1: return y0 + mul_rn(dt, f - mul_rn(a1, third));
    case ODE_RK2: return y0 + mul_rn(dt, (a1 - a2) + f);
    default: return y0 + mul_rn(mul_rn((a1 + mul_rn(3.0f, a2 + a3)) + f, dt), 0.125f);
  }
}

// float4 per thread over B*pitch*mel (a multiple of 4: pitch is a multiple of 128), grid-stride over a grid sized to the CUs.  The stage
// kind is uniform over the launch: each stage touches only the buffers it needs (rk4's last stage: pred x 2, base, k1..k3 in, y out)
__global__ __launch_bounds__(256) void ode_stage_kernel(float* __restrict__ y, const float* __restrict__ pred, size_t total4,
                                                        const OdeStage* __restrict__ stages, const float* __restrict__ cfg_tab,
                                                        const int* __restrict__ step_idx, float* __restrict__ base, float* __restrict__ k1,
                                                        float* __restrict__ k2, float* __restrict__ k3, int use_cfg) {
  const int e = step_idx[0];
  const OdeStage st = stages[e];
  const float cg = cfg_tab[e];
  const int kind = st.kind;
  const bool first = kind == ODE_MID0 || kind == ODE_RK0;
  float4* Y = reinterpret_cast<float4*>(y);
  float4* B0 = reinterpret_cast<float4*>(base);
  float4* K1 = reinterpret_cast<float4*>(k1);
  float4* K2 = reinterpret_cast<float4*>(k2);
  float4* K3 = reinterpret_cast<float4*>(k3);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < total4; v += (size_t)gridDim.x * blockDim.x) {
    const float4 pc = reinterpret_cast<const float4*>(pred)[v];
    float4 f = pc;
    if (use_cfg) {
      const float4 pu = reinterpret_cast<const float4*>(pred)[total4 + v];
      f = make_float4(ode_cfg(pc.x, pu.x, cg), ode_cfg(pc.y, pu.y, cg), ode_cfg(pc.z, pu.z, cg), ode_cfg(pc.w, pu.w, cg));
    }
    float4 y0;
    if (first) { y0 = Y[v]; B0[v] = y0; }
    else y0 = B0[v];
    const float4 a1 = kind >= ODE_RK1 ? K1[v] : z;
    const float4 a2 = kind >= ODE_RK2 ? K2[v] : z;
    const float4 a3 = kind >= ODE_RK3 ? K3[v] : z;
    if (kind == ODE_RK0) K1[v] = f;
    else if (kind == ODE_RK1) K2[v] = f;
    else if (kind == ODE_RK2) K3[v] = f;
    Y[v] = make_float4(ode_stage_elem(kind, st.dt, st.c, f.x, y0.x, a1.x, a2.x, a3.x), ode_stage_elem(kind, st.dt, st.c, f.y, y0.y, a1.y, a2.y, a3.y),
                       ode_stage_elem(kind, st.dt, st.c, f.z, y0.z, a1.z, a2.z, a3.z), ode_stage_elem(kind, st.dt, st.c, f.w, y0.w, a1.w, a2.w, a3.w));
  }
}

// the step counter is advanced by its own 1-thread kernel so that every kernel of step k reads the same value
__global__ void step_advance_kernel(int* step_idx, int value, int set) { step_idx[0] = set ? value : step_idx[0] + 1; }

__global__ void rope_table_kernel(float* __restrict__ cs, float* __restrict__ sn, int n, int half,
                                  const float* __restrict__ inv_freq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * half) return;
  const int pos = i / half, j = i - pos * half;
  const float ang = (float)pos * inv_freq[j];  // fp32 product like einsum('i,j->ij') in the reference
  cs[i] = cosf(ang);
  sn[i] = sinf(ang);
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = (bf16_t)src[i];
}

// conv weight [C_out][Cg (ci)][taps] fp32 -> [G][taps][Cg (co)][Cg (ci)] bf16
__global__ void convpos_weight_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int C, int cg, int taps) {
  const size_t total = (size_t)C * cg * taps;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int tap = (int)(i % taps);
    const int ci = (int)((i / taps) % cg);
    const int cout = (int)(i / ((size_t)taps * cg));
    const int g = cout / cg, co = cout - g * cg;
    dst[(((size_t)g * taps + tap) * cg + co) * cg + ci] = (bf16_t)src[i];
  }
}

// step_cond = where(cond_mask, cond, 0) etc. are host-side one-offs; the final out = where(mask, cond, y):
// `b` lives in the padded row space [B][pitch][cols]; out / a / mask are the caller's dense [B][N][...]
__global__ void select_rows_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b,
                                   const uint8_t* __restrict__ mask, int B, int N, int pitch, int cols) {
  const size_t total = (size_t)B * N * cols;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / cols;
    const int c = (int)(i - row * cols);
    const int bb = (int)(row / N), n = (int)(row - (size_t)bb * N);
    out[i] = mask[row] ? a[i] : b[((size_t)bb * pitch + n) * cols + c];
  }
}

inline int grid_for(size_t n, int block = 256) {
  size_t g = (n + block - 1) / block;
  return (int)(g < 2048 ? (g ? g : 1) : 2048);
}

}  // namespace

hipError_t launch_ln_mod(const float* x, bf16_t* out, int M, int D, const float* tab, int tab_stride, int scale_off,
                         int shift_off, const int* step_idx, hipStream_t s, const int* live_len, int pitch, int batch) {
  if (D != 1024) return hipErrorInvalidValue;
  if (live_len && (pitch <= 0 || pitch % 128 != 0 || batch <= 0)) return hipErrorInvalidValue;
  // two rows per wave: +0.4 ... 1.3 % end to end over one (tools/e2e_ab.py, all three workloads)
  hipLaunchKernelGGL((ln_mod_kernel<1024, 2>), dim3((M + 7) / 8), dim3(256), 0, s, x, out, M, tab, tab_stride, scale_off, shift_off, step_idx,
                     live_len, pitch, batch);
  return hipGetLastError();
}

hipError_t launch_ln_prep(const float* x, bf16_t* xs, float* part, int M, int D, const float* tab, int tab_stride, int scale_off,
                          const int* step_idx, hipStream_t s) {
  if (D != LN_D) return hipErrorInvalidValue;
  hipLaunchKernelGGL((ln_prep_kernel<2>), dim3((M + 7) / 8), dim3(256), 0, s, x, xs, part, M, tab, tab_stride, scale_off, step_idx);
  return hipGetLastError();
}
hipError_t launch_ln_fold_split(const float* tab, int tab_stride, int S, int d, const LnFoldSite* sites, int nsites, bf16_t* A, hipStream_t s) {
  hipLaunchKernelGGL(ln_fold_split_kernel, dim3(S, nsites), dim3(256), 0, s, tab, tab_stride, S, d, sites, A);
  return hipGetLastError();
}
hipError_t launch_ln_fold_combine(const LnFoldSite* sites, int nsites, int max_n, int S, float* tab, int tab_stride, hipStream_t s) {
  hipLaunchKernelGGL(ln_fold_combine_kernel, dim3((max_n + 255) / 256, S, nsites), dim3(256), 0, s, sites, S, tab, tab_stride);
  return hipGetLastError();
}

hipError_t launch_ln_mod_f8(const float* x, uint8_t* out8, uint8_t* mx, int M, int D, const float* tab, int tab_stride,
                            int scale_off, int shift_off, const int* step_idx, hipStream_t s) {
  if (D != 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ln_mod_f8_kernel<1024>, dim3((M + 3) / 4), dim3(256), 0, s, x, out8, mx, M, tab, tab_stride, scale_off,
                     shift_off, step_idx);
  return hipGetLastError();
}

hipError_t launch_mx_quant_rows(const float* x, int M, int K, uint8_t* out8, uint8_t* mx, hipStream_t s) {
  if (K % 32 != 0 || M <= 0) return hipErrorInvalidValue;
  const size_t nt = (size_t)M * (K / 32);
  hipLaunchKernelGGL(mx_quant_rows_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, x, M, K, out8, mx);
  return hipGetLastError();
}

hipError_t launch_w_quant_f8(const float* w, int N, int K, uint8_t* out8, float* scale, hipStream_t s) {
  if (K % 4 != 0 || N <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(w_quant_f8_kernel, dim3((N + 3) / 4), dim3(256), 0, s, w, N, K, out8, scale);
  return hipGetLastError();
}

hipError_t launch_f8_to_bf16(const uint8_t* w8, const float* scale, int N, int K, bf16_t* out, hipStream_t s) {
  if (K % 4 != 0 || N <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(f8_to_bf16_kernel, dim3(grid_for((size_t)N * (K / 4))), dim3(256), 0, s, w8, scale, N, K, out);
  return hipGetLastError();
}

hipError_t launch_cfg_euler(float* y, const float* pred, int rows, int cols, const float* dt_tab, const float* cfg_tab,
                            int* step_idx, float* traj, int use_cfg, hipStream_t s) {
  hipLaunchKernelGGL(cfg_euler_kernel, dim3(grid_for((size_t)rows * cols)), dim3(256), 0, s, y, pred, rows, cols, dt_tab,
                     cfg_tab, step_idx, traj, use_cfg);
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, step_idx, 0, 0);
  return hipGetLastError();
}

hipError_t launch_ode_stage(float* y, const float* pred, int rows, int cols, const OdeStage* stages, const float* cfg_tab, int* step_idx,
                            float* base, float* k1, float* k2, float* k3, int use_cfg, int n_cus, hipStream_t s) {
  const size_t total = (size_t)rows * cols;
  if (total % 4 != 0 || !base) return hipErrorInvalidValue;
  const size_t total4 = total / 4, need = (total4 + 255) / 256, cap = (size_t)(n_cus > 0 ? n_cus : 256) * 2;
  const int grid = (int)(need < cap ? (need ? need : 1) : cap);
  hipLaunchKernelGGL(ode_stage_kernel, dim3(grid), dim3(256), 0, s, y, pred, total4, stages, cfg_tab, step_idx, base, k1, k2, k3, use_cfg);
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, step_idx, 0, 0);
  return hipGetLastError();
}

hipError_t launch_step_set(int* step_idx, int value, hipStream_t s) {
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, step_idx, value, 1);
  return hipGetLastError();
}

hipError_t launch_rope_table(float* cs, float* sn, int n, int half, const float* inv_freq, hipStream_t s) {
  hipLaunchKernelGGL(rope_table_kernel, dim3((n * half + 255) / 256), dim3(256), 0, s, cs, sn, n, half, inv_freq);
  return hipGetLastError();
}

hipError_t launch_f32_to_bf16(const float* src, bf16_t* dst, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, n);
  return hipGetLastError();
}

hipError_t launch_convpos_weight(const float* src, bf16_t* dst, int C, int cg, int taps, hipStream_t s) {
  hipLaunchKernelGGL(convpos_weight_kernel, dim3(grid_for((size_t)C * cg * taps)), dim3(256), 0, s, src, dst, C, cg, taps);
  return hipGetLastError();
}

hipError_t launch_select_rows(float* out, const float* a, const float* b_padded, const uint8_t* mask, int B, int N, int pitch,
                              int cols, hipStream_t s) {
  hipLaunchKernelGGL(select_rows_kernel, dim3(grid_for((size_t)B * N * cols)), dim3(256), 0, s, out, a, b_padded, mask, B, N,
                     pitch, cols);
  return hipGetLastError();
}
