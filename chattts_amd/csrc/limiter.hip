// The look-ahead peak limiter on the device (ctts_peak_limit_ragged): packed float32 segments, every segment limited as if alone, with a
// float32 pre-gain per segment (chattts_amd/limiter.py holds the definition, the condition on the float64 sums and the NumPy twin).
// Per segment at rate fs, W = fs / 100:  u = g x;  r = 1 or T / |u|;  m = the minimum of r over 2 W + 1 samples;  s = the mean of m over
// 2 W + 1 samples (float64 sum, float64 division, one rounding);  y = s u.  A workgroup owns a tile of LM_TILE samples of one segment;
// y may be x, and a tile needs its neighbours' untouched input, so the gain curve s goes through a scratch of 4 bytes per sample:
//  * limiter_init_k  -- the segments' records: the pre-gain, min_gain = 1, both counts 0.
//  * limiter_flag_k  -- per tile, the number of samples with |u| > T: the tile's flag, and by one integer atomic the record's n_over.
//  * limiter_gain_k  -- a tile whose own and adjacent tiles' flags are all zero leaves at once: a halo is 2 W <= 960 < LM_TILE samples,
//    so no sample over T reaches it and s == 1 there by the definition (most tiles of real speech).  Otherwise r of the tile and a halo
//    of 2 W on each side goes to LDS (1 outside the segment), the window minimum is taken in place by doubling -- min is idempotent, two
//    overlapping windows of the largest power of two p <= 2 W + 1 cover it -- each thread holding its 16 values in registers across the
//    barrier between a pass's reads and writes.  The box sum is float64: sums of 32 first, then (2 W + 1) / 32 of those at stride 32
//    and the remainder singly (61 LDS reads per sample, not 961); every partial sum is exact under the condition, so the route does
//    not show in the bits.  s goes to the scratch; min s by an atomic min on the bits (s >= 0) and the count of s < 1 by an integer
//    atomic: neither depends on order, so a record does not depend on what the segment is packed with.
//  * limiter_apply_k -- y = s (g x), or y = g x where the tile left early: 16-byte loads and stores at the pack's own alignment, single
//    samples at a segment's ragged edges.
//
// A STREAM (ctts_peak_limit_stream_step): the segment arrives in pushes.  y[i] depends on x[i - 2 W .. i + 2 W], so with `pos` samples pushed
// before and n_in arriving a step emits samples [e_lo, e_lo + n_out), e_lo = max(0, pos - 2 W), up to pos + n_in - 2 W -- on the last push
// up to the end (limiter.py, stream_plan) -- into a y of its own, never in place, so no curve scratch and no second pass are needed:
//  * limiter_stream_k -- a workgroup owns a tile of LM_TILE emitted samples of one stream and reads the raw samples of tile and halo: from
//    x where the position is at or above pos, from the slot's carry (its last min(pos, 4 W) raw samples) below it, silence outside the
//    signal.  It counts the samples over T in tile and halo in the same pass: with none, y = g x and it leaves (most tiles of real
//    speech); otherwise lm_tile_curve, the body of limiter_gain_k, whence the chunks of a stream, concatenated, are the one-shot
//    limiter's bits however the signal was cut.  The slot's record accumulates over EMITTED samples only: n_over from the tile proper,
//    n_touched and min_gain as in limiter_gain_k, all by order-free atomics; after the last push it is the one-shot record.
//    The descriptor's FIRST workgroup also writes the next carry, samples [pos + n_in - c_out, pos + n_in), into the slot's OTHER buffer
//    (carry [slots][2][LM_CARRY]: a step reads buffer `phase` and writes the other, so the tiles that still read the old carry in this
//    launch never meet the write: no atomics, no waiting); it runs when the step emits nothing, too.
//  * limiter_stream_init_k -- a slot is fresh by its descriptor alone: a descriptor with pos == 0 is a stream's first push (or an empty
//    one before it, when nothing has been counted yet), and its record is set to {g32, 1, 0, 0} by this launch IN FRONT of the step's,
//    on the same stream.  The kernel boundary orders the plain store before every atomic of the step, so nothing races, no host write
//    and no memset is involved, and a slot reused after a close needs no clearing.  The launch is skipped when no descriptor has pos == 0.
#include "common.hpp"
#include "kernels.hpp"

#define LM_T 0x1.c85202p-1f                    // float32(C32 * float32(1 - 2^-22)), C32 = float32(10^(-1 / 20)) = 0x1.c8520ap-1
#define LM_EXT (LM_TILE + 4 * LM_WMAX)         // a tile and its halo of 2 W on each side
#define LM_PER ((LM_EXT + 255) / 256)          // values of the extended tile per thread
static_assert(LM_TILE >= 2 * LM_WMAX && LM_PER == 16, "a halo reaches the adjacent tile only; 16 values per thread");

struct LmStats {        // limiter.STATS
  float g32, min_gain;
  int32_t n_over, n_touched;
};
static_assert(sizeof(LmStats) == 16, "limiter.STATS is 16 bytes");

__device__ __forceinline__ int lm_block_sum(int v, int* red, int tid) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
// whether tile j of a segment of nt tiles computes its gain curve: a sample over T in it or next to it
__device__ __forceinline__ bool lm_active(const int32_t* f, long long j, long long nt) {
  return f[j] != 0 || (j > 0 && f[j - 1] != 0) || (j + 1 < nt && f[j + 1] != 0);
}

__global__ __launch_bounds__(256) void limiter_init_k(const float* __restrict__ gain, LmStats* __restrict__ stats, int n_seg) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_seg) return;
  LmStats st;
  st.g32 = gain[s]; st.min_gain = 1.0f; st.n_over = 0; st.n_touched = 0;
  stats[s] = st;
}

__global__ __launch_bounds__(256) void limiter_flag_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                      const float* __restrict__ gain, int32_t* __restrict__ flags, LmStats* stats) {
  __shared__ int red[4];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long long lo = off[s], n = off[s + 1] - lo, t0 = (long long)blockIdx.x * LM_TILE;
  if (t0 >= n) return;
  const int tl = (int)min((long long)LM_TILE, n - t0);
  const float g = gain[s];
  const float* xt = x + lo + t0;
  float xv[LM_TILE / 256];
#pragma unroll
  for (int i = 0; i < LM_TILE / 256; ++i) {                         // every load in flight before the first is used
    const int k = tid + 256 * i;
    xv[i] = k < tl ? xt[k] : 0.0f;
  }
  int c = 0;
#pragma unroll
  for (int i = 0; i < LM_TILE / 256; ++i) c += fabsf(__fmul_rn(g, xv[i])) > LM_T;
  c = lm_block_sum(c, red, tid);
  if (tid == 0) {
    flags[lo / LM_TILE + s + blockIdx.x] = c;
    if (c) atomicAdd(&stats[s].n_over, c);
  }
}

// The gain curve of one tile, shared by limiter_gain_k and limiter_stream_k.  On entry a[e] = r at position t0 - 2 W + e, e < tl + 4 W
// (written by this workgroup, not yet published: the first barrier is here).  out(k, s) takes the curve of the tile's sample k < tl; the
// record *st gets the tile's min s and its count of s < 1 by atomics.  v: the caller's registers, dead by now.
template <class Out>
__device__ __forceinline__ void lm_tile_curve(float* a, double* q, int* red, float* redf, float (&v)[LM_PER], int tid, int tl, int W, LmStats* st,
                                              Out out) {
  const int L = 2 * W + 1, ext = tl + 4 * W, nm = tl + 2 * W;
  __syncthreads();
  int p = 1;
  for (; 2 * p <= L; p *= 2) {                                    // a[e] = min r over [e, e + p)  ->  over [e, e + 2 p)
#pragma unroll
    for (int i = 0; i < LM_PER; ++i) {
      const int e = tid + 256 * i;
      if (e < ext) v[i] = e + p < ext ? fminf(a[e], a[e + p]) : a[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LM_PER; ++i) {
      const int e = tid + 256 * i;
      if (e < ext) a[e] = v[i];
    }
    __syncthreads();
  }
  // m over [t0 - W, t0 + tl + W): a[e] = min r over [e, e + L), position t0 - W + e;  e + L - p <= nm - 1 + L - p < ext
#pragma unroll
  for (int i = 0; i < LM_PER; ++i) {
    const int e = tid + 256 * i;
    if (e < nm) v[i] = fminf(a[e], a[e + L - p]);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < LM_PER; ++i) {
    const int e = tid + 256 * i;
    if (e < nm) a[e] = v[i];
  }
  __syncthreads();
  for (int e = tid; e + 32 <= nm; e += 256) {                     // q[e] = the sum of m over [e, e + 32)
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 32; ++t) acc += (double)a[e + t];
    q[e] = acc;
  }
  __syncthreads();
  const int nq = L / 32, rem = L % 32;
  const double dL = (double)L;
  float mn = 1.0f;
  int touched = 0;
  for (int k = tid; k < tl; k += 256) {                           // S over [k, k + L): k + 32 (nq - 1) <= nm - 32, k + L - 1 <= nm - 1
    double S = 0.0;
#pragma unroll 8
    for (int j = 0; j < nq; ++j) S += q[k + 32 * j];                // the same order of additions, the loads issued ahead
#pragma unroll 8
    for (int t = 0; t < rem; ++t) S += (double)a[k + 32 * nq + t];
    const float sg = (float)(S / dL);
    out(k, sg);
    mn = fminf(mn, sg);
    touched += sg < 1.0f;
  }
  for (int m = 32; m >= 1; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m, 64));
  if ((tid & 63) == 0) redf[tid >> 6] = mn;
  touched = lm_block_sum(touched, red, tid);                      // its barrier publishes redf as well
  if (tid == 0 && touched) {
    atomicAdd(&st->n_touched, touched);
    atomicMin(reinterpret_cast<unsigned int*>(&st->min_gain), __float_as_uint(fminf(fminf(redf[0], redf[1]), fminf(redf[2], redf[3]))));
  }
}

__global__ __launch_bounds__(256) void limiter_gain_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                      const int32_t* __restrict__ rate, const float* __restrict__ gain,
                                                      const int32_t* __restrict__ flags, float* __restrict__ curve, LmStats* stats) {
  __shared__ float a[LM_EXT];
  __shared__ double q[LM_TILE + 2 * LM_WMAX];
  __shared__ int red[4];
  __shared__ float redf[4];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long long lo = off[s], n = off[s + 1] - lo, t0 = (long long)blockIdx.x * LM_TILE;
  if (t0 >= n) return;
  if (!lm_active(flags + lo / LM_TILE + s, blockIdx.x, (n + LM_TILE - 1) / LM_TILE)) return;
  const int tl = (int)min((long long)LM_TILE, n - t0);
  const int W = rate[s] / 100, ext = tl + 4 * W;
  const float g = gain[s];
  // r over [t0 - 2 W, t0 + tl + 2 W): a[e] is position t0 - 2 W + e
  float v[LM_PER];
#pragma unroll
  for (int i = 0; i < LM_PER; ++i) {                              // every load in flight before the first is used; silence outside
    const int e = tid + 256 * i;
    const long long pos = t0 - 2 * W + e;
    v[i] = (e < ext && pos >= 0 && pos < n) ? x[lo + pos] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < LM_PER; ++i) {
    const int e = tid + 256 * i;
    const float au = fabsf(__fmul_rn(g, v[i]));
    if (e < ext) a[e] = au > LM_T ? __fdiv_rn(LM_T, au) : 1.0f;   // the comparison is false for a NaN: r = 1
  }
  lm_tile_curve(a, q, red, redf, v, tid, tl, W, &stats[s], [&](int k, float sg) { curve[lo + t0 + k] = sg; });
}

__global__ __launch_bounds__(256) void limiter_apply_k(const float* x, float* y, const long long* __restrict__ off,
                                                       const float* __restrict__ gain, const int32_t* __restrict__ flags,
                                                       const float* __restrict__ curve) {
  const int s = blockIdx.y;
  const long long lo = off[s], hi = off[s + 1];
  const long long p = (lo & ~3ll) + ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= hi) return;
  const float g = gain[s];
  const int32_t* f = flags + lo / LM_TILE + s;
  const long long nt = (hi - lo + LM_TILE - 1) / LM_TILE;
  if (p >= lo && p + 4 <= hi) {
    const float4 v = *reinterpret_cast<const float4*>(x + p);
    float u[4] = {__fmul_rn(g, v.x), __fmul_rn(g, v.y), __fmul_rn(g, v.z), __fmul_rn(g, v.w)};
    const long long j0 = (p - lo) / LM_TILE, j1 = (p + 3 - lo) / LM_TILE;
    const bool a0 = lm_active(f, j0, nt), a1 = j1 == j0 ? a0 : lm_active(f, j1, nt);
    if (a0 || a1) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if ((p + c - lo) / LM_TILE == j0 ? a0 : a1) u[c] = __fmul_rn(curve[p + c], u[c]);
    }
    *reinterpret_cast<float4*>(y + p) = make_float4(u[0], u[1], u[2], u[3]);
  } else {
    for (long long k = max(p, lo); k < min(p + 4, hi); ++k) {
      const float u = __fmul_rn(g, x[k]);
      y[k] = lm_active(f, (k - lo) / LM_TILE, nt) ? __fmul_rn(curve[k], u) : u;
    }
  }
}

// ---- streams --------------------------------------------------------------------------------------------------------------------------
static_assert(LM_CARRY == 4 * LM_WMAX && LM_TILE < 65536 / 2 && LM_EXT < 65536, "a slot keeps 4 W samples; two counts share one int");

__device__ __forceinline__ float lm_stream_read(const float* __restrict__ xin, const float* __restrict__ cold, long long g, long long c,
                                                long long pos, long long end) {
  if (g >= pos) return g < end ? xin[g - pos] : 0.0f;
  return g >= c ? cold[g - c] : 0.0f;            // g < c only where g < 0
}

__global__ __launch_bounds__(256) void limiter_stream_init_k(const LmStream* __restrict__ tab, LmStats* __restrict__ stats, int n_streams) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_streams || tab[i].pos != 0) return;
  LmStats st;
  st.g32 = tab[i].gain; st.min_gain = 1.0f; st.n_over = 0; st.n_touched = 0;
  stats[tab[i].slot] = st;
}

__global__ __launch_bounds__(256) void limiter_stream_k(const float* __restrict__ x, const LmStream* __restrict__ tab, float* __restrict__ y,
                                                        float* __restrict__ carry, LmStats* stats) {
  __shared__ float a[LM_EXT];
  __shared__ double q[LM_TILE + 2 * LM_WMAX];
  __shared__ int red[4];
  __shared__ float redf[4];
  const LmStream& D = tab[blockIdx.y];
  const int tid = threadIdx.x;
  const long long n_out = D.n_out, r0 = (long long)blockIdx.x * LM_TILE;   // the tile's first sample, relative to the chunk
  const bool has = r0 < n_out;
  if (!has && blockIdx.x != 0) return;           // the whole workgroup: nothing waits at a barrier
  const long long pos = D.pos, end = pos + D.n_in, c = pos - D.c_in;
  const float* xin = x + D.in_off;
  const float* cold = carry + ((long long)D.slot * 2 + D.phase) * LM_CARRY;
  if (blockIdx.x == 0 && D.total < 0) {          // more to come: keep samples [end - c_out, end); c_out <= LM_CARRY, the host refused the rest
    float* cnew = carry + ((long long)D.slot * 2 + (D.phase ^ 1)) * LM_CARRY;
    const long long nb = end - D.c_out;          // >= c: a carry never reaches back beyond the one before it
    for (int i = tid; i < D.c_out; i += 256) cnew[i] = lm_stream_read(xin, cold, nb + i, c, pos, end);
  }
  if (!has) return;                              // workgroup-uniform
  const int tl = (int)min((long long)LM_TILE, n_out - r0);
  const int W = D.rate / 100, ext = tl + 4 * W;
  const float g = D.gain;
  const long long t0 = D.e_lo + r0;              // the tile's first sample, in the signal
  // r over [t0 - 2 W, t0 + tl + 2 W): a[e] is position t0 - 2 W + e; on a push that is not the last, t0 + tl + 2 W <= end
  float v[LM_PER];
#pragma unroll
  for (int i = 0; i < LM_PER; ++i) {             // every load in flight before the first is used; silence outside the signal
    const int e = tid + 256 * i;
    v[i] = e < ext ? lm_stream_read(xin, cold, t0 - 2 * W + e, c, pos, end) : 0.0f;
  }
  int cnt = 0;                                   // samples over T: of the tile in the low half, of tile and halo in the high half
#pragma unroll
  for (int i = 0; i < LM_PER; ++i) {
    const int e = tid + 256 * i;
    const float au = fabsf(__fmul_rn(g, v[i]));
    const bool over = au > LM_T;                 // false for a NaN: r = 1
    if (e < ext) {
      a[e] = over ? __fdiv_rn(LM_T, au) : 1.0f;
      cnt += over ? 65536 + (e >= 2 * W && e < 2 * W + tl) : 0;
    }
  }
  cnt = lm_block_sum(cnt, red, tid);
  LmStats* st = stats + D.slot;
  if (tid == 0 && (cnt & 65535)) atomicAdd(&st->n_over, cnt & 65535);
  float* yw = y + D.out_off + r0;
  if (cnt == 0) {                                // nothing over T in reach: s == 1 on the whole tile, y = u
#pragma unroll
    for (int i = 0; i < LM_PER; ++i) {
      const int k = tid + 256 * i - 2 * W;
      if (k >= 0 && k < tl) yw[k] = __fmul_rn(g, v[i]);
    }
    return;
  }
  lm_tile_curve(a, q, red, redf, v, tid, tl, W, st,
                [&](int k, float sg) { yw[k] = __fmul_rn(sg, __fmul_rn(g, lm_stream_read(xin, cold, t0 + k, c, pos, end))); });
}

hipError_t launch_peak_limit_stream(const float* x, const LmStream* tab, int n_streams, long long n_out_max, float* y, float* carry,
                                    void* stats, int reset, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  if (reset) {
    hipLaunchKernelGGL(limiter_stream_init_k, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, st, tab, (LmStats*)stats, n_streams);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // at least one workgroup per descriptor: a step that emits nothing still appends its push to the carry
  const long long tiles = (n_out_max + LM_TILE - 1) / LM_TILE;
  hipLaunchKernelGGL(limiter_stream_k, dim3((unsigned)(tiles > 0 ? tiles : 1), (unsigned)n_streams), dim3(256), 0, st, x, tab, y, carry,
                     (LmStats*)stats);
  return hipGetLastError();
}

hipError_t launch_peak_limit_ragged(const float* x, float* y, const long long* off, int n_seg, long long n_max, const int32_t* rate,
                                    const float* gain, void* stats, float* curve, int32_t* flags, hipStream_t st) {
  if (n_seg <= 0 || n_max <= 0) return hipSuccess;
  hipLaunchKernelGGL(limiter_init_k, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, st, gain, (LmStats*)stats, n_seg);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 gt((unsigned)((n_max + LM_TILE - 1) / LM_TILE), (unsigned)n_seg);
  hipLaunchKernelGGL(limiter_flag_k, gt, dim3(256), 0, st, x, off, gain, flags, (LmStats*)stats);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(limiter_gain_k, gt, dim3(256), 0, st, x, off, rate, gain, flags, curve, (LmStats*)stats);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 ga((unsigned)((n_max + 3 + 1023) / 1024), (unsigned)n_seg);
  hipLaunchKernelGGL(limiter_apply_k, ga, dim3(256), 0, st, x, y, off, gain, flags, curve);
  return hipGetLastError();
}
