// Loudness normalisation on the device (ctts_loudness_normalize_ragged): ITU-R BS.1770-4 integrated loudness of packed float32 segments,
// every segment filtered as if alone, ONE loudness and ONE float32 gain per group of segments (chattts_amd/loudness.py holds the definition
// and the host side).  The K-weighting is two biquads in cascade, a 4-state linear system s' = A s + B x, y = C s + D x (ln_step is one
// sample of it, transposed direct form II, float64 throughout).  A 10 s segment is a 240,000-step chain; it is computed exactly and in
// parallel in three launches:
//  * loudness_tile_k -- one wave per tile of H = fs / 10 samples (a 100 ms sub-block; a segment's last tile may be partial), four tiles per
//    workgroup (two above H = 4096), staged in LDS by coalesced loads (the peak rides along; 4 H floats, sized by the call's largest H).  Lane l owns the chunk
//    [l c, (l + 1) c), c = ceil(H / 64) | 1 -- odd, so the lanes' reads at stride c fall on 32 different banks:
//      A  it runs its chunk from zero state -> z_l;
//      -  six shuffle steps scan the chunks' states with A^(c 2^k) (host table): lane l's entry state under a zero tile entry;
//      B  it runs its chunk again from that state -> y0_i, the tile's outputs under zero entry, and next to it the system WITHOUT input
//         from the four columns of A^(l c) (host table), whose outputs are h_i = C A^i at the lane's positions.  It sums y0_i^2, y0_i h_i
//         and, in a partial tile only, h_i h_i^T (a full tile's M = sum h_i h_i^T is in the host table).
//    A butterfly adds the lanes' sums in a fixed order; lane 0 writes the tile's record: z[4] (end state), e0, v[4], M[10], peak.
//  * loudness_group_k -- one workgroup per group.  Per segment, in batches of 256 tiles: the end states go to LDS, thread 0 chains the
//    true entry states s_{j+1} = A^H s_j + z_j, and every thread corrects its tile's energy in closed form,
//    e_j = e0_j + 2 s_j . v_j + s_j^T M s_j.  Then the blocks z_i = (e_i + .. + e_{i+3}) / (4 H) (a segment with fewer than four complete
//    sub-blocks: one block, its mean square) pass the absolute gate and the relative gate -- thread t takes blocks t, t + 256, .. of every
//    segment, and the threads' sums go through one LDS tree: the order depends on the group alone, never on the pack.  Thread 0 computes L,
//    the gain and the record; the group's gain goes to every one of its segments.
//  * loudness_scale_k -- y = g32 * x over the pack, one rounding per sample: 16-byte loads and stores at the pack's own alignment, single
//    samples at a segment's ragged edges.  y may be x.
// With a limiter table (ctts_loudness_limited_ragged) a flagged group's gain drops the ceiling term -- the peak limiter behind this stage
// (limiter.hip) enforces it -- its segments are left unscaled, and every segment's gain goes where that call reads it.
#include "common.hpp"
#include "kernels.hpp"

#define LN_LN10_ABS 1.1724653045822964e-07     // 10^((-70 + 0.691) / 10): l_i > -70  <=>  z_i > this
#define LN_MAX_GAIN 31.622776601683793         // 10^(30 / 20)
#define LN_CEILING 0.8912509381337456          // 10^(-1 / 20)

struct LnStats {        // loudness.STATS
  double L;
  float peak, g32;
  int32_t n_blocks, n_abs, n_rel, bound;
};
static_assert(sizeof(LnStats) == 32, "loudness.STATS is 32 bytes");

// one sample of the cascade; k: b0 b1 b2 a1 a2 of the shelf, then of the high-pass
__device__ __forceinline__ double ln_step(const double* k, double x, double& s0, double& s1, double& s2, double& s3) {
  const double y1 = fma(k[0], x, s0);
  s0 = fma(-k[3], y1, fma(k[1], x, s1));
  s1 = fma(-k[4], y1, k[2] * x);
  const double y2 = fma(k[5], y1, s2);
  s2 = fma(-k[8], y2, fma(k[6], y1, s3));
  s3 = fma(-k[9], y2, k[7] * y1);
  return y2;
}
// the same without input
__device__ __forceinline__ double ln_step0(const double* k, double& s0, double& s1, double& s2, double& s3) {
  const double y1 = s0;
  s0 = fma(-k[3], y1, s1);
  s1 = -k[4] * y1;
  const double y2 = fma(k[5], y1, s2);
  s2 = fma(-k[8], y2, fma(k[6], y1, s3));
  s3 = fma(-k[9], y2, k[7] * y1);
  return y2;
}
__device__ __forceinline__ double ln_wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(64 * LN_WAVES) void loudness_tile_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                                 const int32_t* __restrict__ rate, const double* __restrict__ coef,
                                                                 double* __restrict__ rec, int h_max) {
  extern __shared__ __align__(16) float ln_tile[];                 // one tile of h_max floats per wave of the workgroup
  const int s = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const long long lo = off[s], n = off[s + 1] - lo;
  const double* R = coef + (long long)rate[s] * LN_ROW;
  const int H = (int)R[0], c = (int)R[1];
  const long long j = (long long)blockIdx.x * (blockDim.x >> 6) + w;   // this wave's tile of the segment
  const long long t0 = j * H;
  const int tl = t0 < n ? (int)min((long long)H, n - t0) : 0;    // 0: no such tile
  float* tw = ln_tile + w * h_max;
  float pk = 0.0f;
  for (int i = l; i < tl; i += 64) {
    const float v = x[lo + t0 + i];
    tw[i] = v;
    pk = fmaxf(pk, fabsf(v));
  }
  __syncthreads();                                                // the only barrier: a wave without a tile leaves behind it
  if (tl == 0) return;
  double k[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) k[i] = R[2 + i];
  const int st = l * c, len = max(0, min(c, tl - st));
  // A: the chunk from zero state
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int i = 0; i < len; ++i) ln_step(k, (double)tw[st + i], s0, s1, s2, s3);
  // inclusive scan S_l = sum_{m <= l} A^(c (l - m)) z_m.  Every lane in front of the last one with samples ran a full chunk, so its S is
  // the state behind its chunk; what the lanes from that one on hold is never read
  const double* P = R + 48;
  for (int d = 1; d < 64; d <<= 1) {
    const double* Pd = P + d * 16;
    const double u0 = __shfl_up(s0, d, 64), u1 = __shfl_up(s1, d, 64), u2 = __shfl_up(s2, d, 64), u3 = __shfl_up(s3, d, 64);
    if (l >= d) {
      s0 += Pd[0] * u0 + Pd[1] * u1 + Pd[2] * u2 + Pd[3] * u3;
      s1 += Pd[4] * u0 + Pd[5] * u1 + Pd[6] * u2 + Pd[7] * u3;
      s2 += Pd[8] * u0 + Pd[9] * u1 + Pd[10] * u2 + Pd[11] * u3;
      s3 += Pd[12] * u0 + Pd[13] * u1 + Pd[14] * u2 + Pd[15] * u3;
    }
  }
  s0 = __shfl_up(s0, 1, 64); s1 = __shfl_up(s1, 1, 64); s2 = __shfl_up(s2, 1, 64); s3 = __shfl_up(s3, 1, 64);
  if (l == 0) s0 = s1 = s2 = s3 = 0.0;
  // B: the chunk from its entry state, and the four unit states' responses from A^(l c)
  const double* Pl = P + l * 16;
  double g[4][4];                                                 // g[q][r]: state r of the run that started at unit state q
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) g[q][r] = Pl[r * 4 + q];
  const bool part = tl < H;
  double e = 0.0, v[4] = {0.0, 0.0, 0.0, 0.0}, M[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < len; ++i) {
    const double y = ln_step(k, (double)tw[st + i], s0, s1, s2, s3);
    double h[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q] = ln_step0(k, g[q][0], g[q][1], g[q][2], g[q][3]);
    e = fma(y, y, e);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = fma(y, h[q], v[q]);
    if (part) {
      int m = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = q; r < 4; ++r) { M[m] = fma(h[q], h[r], M[m]); ++m; }
    }
  }
  const int la = (tl - 1) / c;                                    // the lane that holds the tile's end state
  const double z0 = __shfl(s0, la, 64), z1 = __shfl(s1, la, 64), z2 = __shfl(s2, la, 64), z3 = __shfl(s3, la, 64);
  e = ln_wave_sum(e);
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = ln_wave_sum(v[q]);
  if (part) {
#pragma unroll
    for (int m = 0; m < 10; ++m) M[m] = ln_wave_sum(M[m]);
  }
  for (int m = 32; m >= 1; m >>= 1) pk = fmaxf(pk, __shfl_xor(pk, m, 64));
  if (l == 0) {
    double* r = rec + (lo / LN_HMIN + s + j) * LN_REC;
    r[0] = z0; r[1] = z1; r[2] = z2; r[3] = z3;
    r[4] = e;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[5 + q] = v[q];
#pragma unroll
    for (int m = 0; m < 10; ++m) r[9 + m] = M[m];
    r[19] = (double)pk;
  }
}

// the block's sum of v in a fixed order (a tree over the threads), the same in every thread
__device__ __forceinline__ double ln_block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if (tid < m) red[tid] += red[tid + m];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// f(z) for the blocks of the group's segments that fall to this thread: block i of a segment to thread i mod 256
template <class F>
__device__ __forceinline__ void ln_for_blocks(const long long* off, const int32_t* rate, const double* coef, const double* rec, int sa, int sb,
                                              int tid, F f) {
  for (int s = sa; s < sb; ++s) {
    const long long lo = off[s], n = off[s + 1] - lo;
    const int H = (int)coef[(long long)rate[s] * LN_ROW];
    const double* r = rec + (lo / LN_HMIN + s) * LN_REC;
    const long long nb = n / H;
    if (nb >= 4) {
      const double d = 4.0 * H;
      for (long long i = tid; i < nb - 3; i += 256)
        f((r[i * LN_REC + 4] + r[(i + 1) * LN_REC + 4] + r[(i + 2) * LN_REC + 4] + r[(i + 3) * LN_REC + 4]) / d);
    } else if (tid == 0) {
      const int nt = (int)((n + H - 1) / H);                      // at most 4
      double a = 0.0;
      for (int i = 0; i < nt; ++i) a += r[i * LN_REC + 4];
      f(a / (double)n);
    }
  }
}

__global__ __launch_bounds__(256) void loudness_group_k(const long long* __restrict__ off, const int32_t* __restrict__ rate,
                                                        const double* __restrict__ coef, const int32_t* __restrict__ grp,
                                                        const double* __restrict__ target, double* rec, float* __restrict__ seg_gain,
                                                        LnStats* __restrict__ stats, const int32_t* __restrict__ lim,
                                                        float* __restrict__ gain_out) {
  __shared__ double zs[256][4];
  __shared__ double red[256];
  __shared__ float gsh;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int sa = grp[g], sb = grp[g + 1];
  float pk = 0.0f;
  for (int s = sa; s < sb; ++s) {
    const long long lo = off[s], n = off[s + 1] - lo;
    const double* R = coef + (long long)rate[s] * LN_ROW;
    const int H = (int)R[0];
    const long long nt = (n + H - 1) / H;
    double* rs = rec + (lo / LN_HMIN + s) * LN_REC;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;                // thread 0: the entry state of the next tile
    for (long long b = 0; b < nt; b += 256) {
      const long long j = b + tid;
      double* rj = rs + j * LN_REC;
      if (j < nt) {
        zs[tid][0] = rj[0]; zs[tid][1] = rj[1]; zs[tid][2] = rj[2]; zs[tid][3] = rj[3];
        pk = fmaxf(pk, (float)rj[19]);
      }
      __syncthreads();
      if (tid == 0) {
        const int m = (int)min(256ll, nt - b);
        for (int i = 0; i < m; ++i) {
          const double z0 = zs[i][0], z1 = zs[i][1], z2 = zs[i][2], z3 = zs[i][3];
          zs[i][0] = c0; zs[i][1] = c1; zs[i][2] = c2; zs[i][3] = c3;
          const double n0 = R[16] * c0 + R[17] * c1 + R[18] * c2 + R[19] * c3 + z0;
          const double n1 = R[20] * c0 + R[21] * c1 + R[22] * c2 + R[23] * c3 + z1;
          const double n2 = R[24] * c0 + R[25] * c1 + R[26] * c2 + R[27] * c3 + z2;
          const double n3 = R[28] * c0 + R[29] * c1 + R[30] * c2 + R[31] * c3 + z3;
          c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        }
      }
      __syncthreads();
      if (j < nt) {
        const double a0 = zs[tid][0], a1 = zs[tid][1], a2 = zs[tid][2], a3 = zs[tid][3];
        const double* M = (n - j * H >= H) ? R + 32 : rj + 9;     // a full tile's M is the rate's
        const double lin = a0 * rj[5] + a1 * rj[6] + a2 * rj[7] + a3 * rj[8];
        const double quad = a0 * (M[0] * a0 + 2.0 * (M[1] * a1 + M[2] * a2 + M[3] * a3)) + a1 * (M[4] * a1 + 2.0 * (M[5] * a2 + M[6] * a3)) +
                            a2 * (M[7] * a2 + 2.0 * M[8] * a3) + a3 * M[9] * a3;
        rj[4] = rj[4] + 2.0 * lin + quad;
      }
      __syncthreads();                                            // the next batch overwrites zs; the energies are visible to the block
    }
  }
  // the absolute gate
  double cnt = 0.0, cnt_abs = 0.0, sum_abs = 0.0;
  ln_for_blocks(off, rate, coef, rec, sa, sb, tid, [&](double z) {
    cnt += 1.0;
    if (z > LN_LN10_ABS) { cnt_abs += 1.0; sum_abs += z; }
  });
  cnt = ln_block_sum(cnt, red, tid);
  cnt_abs = ln_block_sum(cnt_abs, red, tid);
  sum_abs = ln_block_sum(sum_abs, red, tid);
  // the relative gate, 10 LU under the mean of what passed: l_i > G  <=>  z_i > mean / 10
  const double thr = cnt_abs > 0.0 ? 0.1 * (sum_abs / cnt_abs) : 0.0;
  double cnt_rel = 0.0, sum_rel = 0.0;
  ln_for_blocks(off, rate, coef, rec, sa, sb, tid, [&](double z) {
    if (z > LN_LN10_ABS && z > thr) { cnt_rel += 1.0; sum_rel += z; }
  });
  cnt_rel = ln_block_sum(cnt_rel, red, tid);
  sum_rel = ln_block_sum(sum_rel, red, tid);
  red[tid] = (double)pk;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if (tid < m) red[tid] = fmax(red[tid], red[tid + m]);
    __syncthreads();
  }
  const bool limited = lim && lim[g] != 0;                        // the limiter behind this stage enforces the ceiling
  if (tid == 0) {
    const float peak = (float)red[0];
    const double t = target[g];
    double L = -INFINITY, gain = 1.0;
    int bound = -1;
    if (cnt_abs > 0.0) {
      L = -0.691 + 10.0 * log10(sum_rel / cnt_rel);
      if (t == t) {                                               // NaN: the group is measured and left alone
        gain = pow(10.0, (t - L) / 20.0);
        bound = 0;
        if (LN_MAX_GAIN < gain) { gain = LN_MAX_GAIN; bound = 1; }
        const double ceil_g = LN_CEILING / (double)peak;
        if (!limited && ceil_g < gain) { gain = ceil_g; bound = 2; }
      }
    }
    LnStats st;
    st.L = L; st.peak = peak; st.g32 = (float)gain;
    st.n_blocks = (int32_t)cnt; st.n_abs = (int32_t)cnt_abs; st.n_rel = (int32_t)cnt_rel; st.bound = bound;
    stats[g] = st;
    gsh = st.g32;
  }
  __syncthreads();
  const float g32 = gsh;
  for (int s = sa + tid; s < sb; s += 256) {
    seg_gain[s] = limited ? 1.0f : g32;                           // the limiter applies the gain itself: the scale pass leaves x as it is
    if (gain_out) gain_out[s] = g32;
  }
}

__global__ __launch_bounds__(256) void loudness_scale_k(const float* x, float* y, const long long* __restrict__ off,
                                                        const float* __restrict__ seg_gain, int skip_unity) {
  const int s = blockIdx.y;
  const long long lo = off[s], hi = off[s + 1];
  const long long p = (lo & ~3ll) + ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= hi) return;
  const float g = seg_gain[s];
  if (skip_unity && g == 1.0f && x == y) return;                  // a segment that waits for the limiter, in place: nothing to do
  if (p >= lo && p + 4 <= hi) {
    const float4 v = *reinterpret_cast<const float4*>(x + p);
    *reinterpret_cast<float4*>(y + p) = make_float4(__fmul_rn(g, v.x), __fmul_rn(g, v.y), __fmul_rn(g, v.z), __fmul_rn(g, v.w));
  } else {
    for (long long q = max(p, lo); q < min(p + 4, hi); ++q) y[q] = __fmul_rn(g, x[q]);
  }
}

hipError_t launch_loudness_normalize_ragged(const float* x, float* y, const long long* off, int n_seg, long long n_max, long long tiles_max,
                                            int h_max, const int32_t* rate, const double* coef, const int32_t* grp, int n_grp, const double* target,
                                            void* stats, double* rec, float* seg_gain, hipStream_t st, const int32_t* lim, float* gain_out) {
  if (n_seg <= 0 || n_grp <= 0 || n_max <= 0 || h_max < LN_HMIN || h_max > LN_HMAX) return hipSuccess;
  // LN_WAVES tiles per workgroup where they fit the 64 KB of LDS a launch gets without asking for more (H <= 4096), else half as many
  const int waves = (size_t)LN_WAVES * h_max * sizeof(float) <= 65536 ? LN_WAVES : LN_WAVES / 2;
  const dim3 g1((unsigned)((tiles_max + waves - 1) / waves), (unsigned)n_seg);
  hipLaunchKernelGGL(loudness_tile_k, g1, dim3(64 * waves), (size_t)waves * h_max * sizeof(float), st, x, off, rate, coef, rec, h_max);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loudness_group_k, dim3((unsigned)n_grp), dim3(256), 0, st, off, rate, coef, grp, target, rec, seg_gain, (LnStats*)stats, lim,
                     gain_out);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 g3((unsigned)((n_max + 3 + 1023) / 1024), (unsigned)n_seg);
  hipLaunchKernelGGL(loudness_scale_k, g3, dim3(256), 0, st, x, y, off, seg_gain, lim ? 1 : 0);
  return hipGetLastError();
}
