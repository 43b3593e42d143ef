// Pitch-preserving time scaling on the device (ctts_time_scale_ragged): waveform-similarity overlap-add (WSOLA) at 24 kHz over packed
// segments, the layout the ragged decoder writes.  Every segment is scaled as if alone: positions outside its own [0, n) read as zero.
//   N = TS_N = 1024 (window), HS = TS_HS = 512 (synthesis hop), D = TS_D = 256 (search radius), w[j] = 0.5 - 0.5 cos(2 pi j / N)
//   speed = num / den:  n_out = ceil(n den / num),  F = ceil(n_out / HS) + 1 frames,  a_k = floor(k HS num / den),  s_0 = -HS
//   k >= 1:  t[j] = x[s_{k-1} + HS + j],  c(d) = sum_{j<N} t[j] x[a_k - HS + d + j],  d in [-D, D)
//            d_k = arg max c (equal c: the smallest |d|, then the negative one),  s_k = a_k - HS + d_k
//   y[(k-1) HS + j] = w[j + HS] x[s_{k-1} + HS + j] + w[j] x[s_k + j],  0 <= j < HS          (w[j] + w[j + HS] = 1: nothing to normalise)
// (chattts_amd/timescale.py is the host side.)  Two launches:
//  * timescale_path_k -- the search is a chain (s_k needs s_{k-1}), so ONE workgroup walks a segment's frames; the segments of a pack run
//    side by side.  A frame stages the template (1024 floats) and the span x[a_k - HS - D .. a_k - HS + D + N - 1) (1535 floats) in LDS,
//    10 KB.  Thread q of 256 owns candidates 2q and 2q + 1: per two taps it reads one aligned float2 of the span (lanes on consecutive
//    float2s: conflict-free) and the template as a broadcast float4 per four taps -- four FMAs per span read.  A candidate's sum is two
//    chains (even and odd taps, j ascending) added once; the order is fixed, so a path never depends on the pack.  The arg-max goes
//    through the wave (shuffles) and four LDS slots under ONE total order that carries the tie rule, hence any reduction order gives the
//    same winner, and a frame whose products are all zero gets d = 0.
//  * timescale_ola_k -- the overlap-add needs the finished path only: one thread per output sample over the whole pack, two masked loads,
//    two products and one sum, each rounded (no contraction): what timescale.apply computes in NumPy float32.
// Streams (ctts_time_scale_stream_step): the signal arrives in pushes, the output leaves in chunks, and their concatenation is the one-shot
// result bit for bit.  One launch:
//  * timescale_stream_k -- one workgroup per stream walks the frames (k_prev, k_now] that the push made final (the host's arithmetic:
//    timescale.stream_plan).  A read at stream position g comes from the new samples (g >= pos), from the slot's carry x[base(k_prev), pos)
//    or is zero (g < 0, or g >= total on the last push).  The search is ts_search_frame, the function timescale_path_k runs, over the same
//    staging; the overlap-add of frame k needs x[s_{k-1} + HS + j] = tpl[j] and x[s_k + j] = sp[d_k + D + j], both still in LDS, so the
//    same workgroup writes y[(k - 1) HS + j] with timescale_ola_k's two products and one sum.  Then it writes x[base(k_now), pos + n_in)
//    into the slot's OTHER carry buffer (the step reads one and writes the other: no copy in place) and s_{k_now} into the slot's state.
#include "common.hpp"
#include "kernels.hpp"

#define TS_SPAN (2 * TS_D + TS_N)   // 1536: the span's 1535 floats and one zero

// (c1, d1) before (c2, d2) in the search's order
__device__ __forceinline__ bool ts_better(float c1, int d1, float c2, int d2) {
  if (c1 != c2) return c1 > c2;
  const int m1 = d1 < 0 ? -d1 : d1, m2 = d2 < 0 ? -d2 : d2;
  return m1 != m2 ? m1 < m2 : d1 < d2;
}

// The search of one frame over the staged template and span, shared by the one-shot and the streaming kernel: d_k, the same in every
// thread.  Two barriers: staging -> sums, the waves' slots -> the winner; the caller's own barrier frees tpl / sp / red for the next frame.
__device__ __forceinline__ int ts_search_frame(const float* tpl, const float* sp, float* red_c, int* red_d, int tid) {
  __syncthreads();
  // candidates 2 tid and 2 tid + 1: c(d) = sum_j tpl[j] sp[d + D + j]
  const float2* sv = reinterpret_cast<const float2*>(sp) + tid;
  const float4* tv = reinterpret_cast<const float4*>(tpl);
  float a0e = 0.0f, a0o = 0.0f, a1e = 0.0f, a1o = 0.0f;
  float2 v0 = sv[0];
#pragma unroll 4
  for (int j = 0; j < TS_N / 4; ++j) {
    const float4 t = tv[j];
    const float2 v1 = sv[2 * j + 1];
    const float2 v2 = sv[2 * j + 2];           // float2 tid + 2 j + 2 <= 255 + 512 = TS_SPAN / 2 - 1: the last one holds span[1534] and the zero
    a0e = fmaf(t.x, v0.x, a0e);
    a0o = fmaf(t.y, v0.y, a0o);
    a1e = fmaf(t.x, v0.y, a1e);
    a1o = fmaf(t.y, v1.x, a1o);
    a0e = fmaf(t.z, v1.x, a0e);
    a0o = fmaf(t.w, v1.y, a0o);
    a1e = fmaf(t.z, v1.y, a1e);
    a1o = fmaf(t.w, v2.x, a1o);
    v0 = v2;
  }
  const float c0 = a0e + a0o, c1 = a1e + a1o;
  const int d0 = 2 * tid - TS_D, d1 = d0 + 1;
  float bc = c0;
  int bd = d0;
  if (ts_better(c1, d1, bc, bd)) { bc = c1; bd = d1; }
  for (int m = 32; m >= 1; m >>= 1) {
    const float oc = __shfl_xor(bc, m, 64);
    const int od = __shfl_xor(bd, m, 64);
    if (ts_better(oc, od, bc, bd)) { bc = oc; bd = od; }
  }
  if ((tid & 63) == 0) { red_c[tid >> 6] = bc; red_d[tid >> 6] = bd; }
  __syncthreads();
  bc = red_c[0];
  bd = red_d[0];
  for (int w = 1; w < 4; ++w)
    if (ts_better(red_c[w], red_d[w], bc, bd)) { bc = red_c[w]; bd = red_d[w]; }
  return bd;
}

__global__ __launch_bounds__(256) void timescale_path_k(const float* __restrict__ x, const long long* __restrict__ off_in,
                                                        const long long* __restrict__ off_out, int32_t* __restrict__ path,
                                                        const long long* __restrict__ path_off, int num, int den) {
  __shared__ __align__(16) float tpl[TS_N];
  __shared__ __align__(16) float sp[TS_SPAN];
  __shared__ float red_c[4];
  __shared__ int red_d[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long lo = off_in[s], n = off_in[s + 1] - lo, n_out = off_out[s + 1] - off_out[s];
  const int F = (int)((n_out + TS_HS - 1) / TS_HS) + 1;
  int32_t* ps = path + path_off[s];
  const float* xs = x + lo;
  long long s_prev = -TS_HS;
  if (tid == 0) ps[0] = -TS_HS;
  for (int k = 1; k < F; ++k) {
    const long long a = (long long)k * TS_HS * num / den;
    const long long t0 = s_prev + TS_HS, b0 = a - TS_HS - TS_D;
    for (int e = tid; e < TS_N; e += 256) {
      const long long g = t0 + e;
      tpl[e] = (g >= 0 && g < n) ? xs[g] : 0.0f;
    }
    for (int e = tid; e < TS_SPAN; e += 256) {
      const long long g = b0 + e;
      sp[e] = (e < TS_SPAN - 1 && g >= 0 && g < n) ? xs[g] : 0.0f;
    }
    const int bd = ts_search_frame(tpl, sp, red_c, red_d, tid);
    s_prev = a - TS_HS + bd;                     // every thread holds the same winner
    if (tid == 0) ps[k] = (int32_t)s_prev;
    __syncthreads();                             // the next frame overwrites tpl / sp / red
  }
}

__global__ __launch_bounds__(256) void timescale_ola_k(const float* __restrict__ x, const long long* __restrict__ off_in, float* __restrict__ y,
                                                       const long long* __restrict__ off_out, const int32_t* __restrict__ path,
                                                       const long long* __restrict__ path_off, const float* __restrict__ window) {
  const int s = blockIdx.y;
  const long long lo = off_in[s], n = off_in[s + 1] - lo;
  const long long olo = off_out[s], n_out = off_out[s + 1] - olo;
  const long long m = (long long)blockIdx.x * TS_TILE + threadIdx.x * 4ll;
  if (m >= n_out) return;
  const int32_t* ps = path + path_off[s];
  const float* xs = x + lo;
  const long long k1 = m / TS_HS;                // frame k - 1; four consecutive samples from a multiple of 4 share it
  const long long sa = (long long)ps[k1] + TS_HS, sb = ps[k1 + 1];
  const int j0 = (int)(m - k1 * TS_HS);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (m + i >= n_out) break;
    const int j = j0 + i;
    const long long ga = sa + j, gb = sb + j;
    const float xa = (ga >= 0 && ga < n) ? xs[ga] : 0.0f, xb = (gb >= 0 && gb < n) ? xs[gb] : 0.0f;
    y[olo + m + i] = __fadd_rn(__fmul_rn(window[j + TS_HS], xa), __fmul_rn(window[j], xb));
  }
}

__device__ __forceinline__ float ts_stream_read(const float* __restrict__ xin, const float* __restrict__ carry, long long g, long long base,
                                                long long pos, long long end) {
  if (g >= pos) return g < end ? xin[g - pos] : 0.0f;
  return g >= base ? carry[g - base] : 0.0f;
}

__global__ __launch_bounds__(256) void timescale_stream_k(const float* __restrict__ x, const TsStream* __restrict__ tab, float* __restrict__ y,
                                                          int32_t* __restrict__ path, float* __restrict__ carry, int32_t* __restrict__ state,
                                                          const float* __restrict__ window) {
  __shared__ __align__(16) float tpl[TS_N];
  __shared__ __align__(16) float sp[TS_SPAN];
  __shared__ float red_c[4];
  __shared__ int red_d[4];
  const int tid = threadIdx.x;
  const TsStream w = tab[blockIdx.x];
  const int num = w.num, den = w.den;
  const float* xin = x + w.in_off;
  const float* cold = carry + ((long long)w.slot * 2 + w.phase) * TS_CARRY;
  float* cnew = carry + ((long long)w.slot * 2 + (w.phase ^ 1)) * TS_CARRY;
  const long long pos = w.pos, end = pos + w.n_in;
  const long long base = max(0ll, (long long)w.k_prev * TS_HS * num / den - TS_HS - TS_D);
  long long s_prev = w.k_prev == 0 ? -TS_HS : (long long)state[w.slot * TS_STATE_INTS];
  int32_t* ps = path + w.path_off;
  if (w.k_prev == 0 && w.k_now > 0) {            // s_0 goes out with frame 1
    if (tid == 0) ps[0] = -TS_HS;
    ++ps;
  }
  const float w0 = window[tid], w1 = window[tid + 256], w2 = window[tid + TS_HS], w3 = window[tid + TS_HS + 256];
  float* ys = y + w.out_off;
  for (int k = w.k_prev + 1; k <= w.k_now; ++k) {
    const long long a = (long long)k * TS_HS * num / den;
    const long long t0 = s_prev + TS_HS, b0 = a - TS_HS - TS_D;
    for (int e = tid; e < TS_N; e += 256) tpl[e] = ts_stream_read(xin, cold, t0 + e, base, pos, end);
    for (int e = tid; e < TS_SPAN; e += 256) sp[e] = e < TS_SPAN - 1 ? ts_stream_read(xin, cold, b0 + e, base, pos, end) : 0.0f;
    const int bd = ts_search_frame(tpl, sp, red_c, red_d, tid);
    s_prev = a - TS_HS + bd;
    if (tid == 0) ps[k - w.k_prev - 1] = (int32_t)s_prev;
    // samples [(k - 1) HS, k HS) of the stream = [m0, m0 + HS) of this chunk; only the last chunk ends inside a frame
    const int m0 = (k - w.k_prev - 1) * TS_HS;
    if (m0 + tid < w.n_out) ys[m0 + tid] = __fadd_rn(__fmul_rn(w2, tpl[tid]), __fmul_rn(w0, sp[bd + TS_D + tid]));
    if (m0 + tid + 256 < w.n_out) ys[m0 + tid + 256] = __fadd_rn(__fmul_rn(w3, tpl[tid + 256]), __fmul_rn(w1, sp[bd + TS_D + tid + 256]));
    __syncthreads();                             // the next frame overwrites tpl / sp / red
  }
  if (tid == 0) state[w.slot * TS_STATE_INTS] = (int32_t)s_prev;
  if (w.total < 0) {                             // more to come: keep x[base(k_now), end)
    const long long nb = max(0ll, (long long)w.k_now * TS_HS * num / den - TS_HS - TS_D);
    const int len = (int)(end - nb);             // <= TS_CARRY: the host refused anything else
    for (int i = tid; i < len; i += 256) cnew[i] = ts_stream_read(xin, cold, nb + i, base, pos, end);
  }
}

hipError_t launch_time_scale_stream(const float* x, const TsStream* tab, int n_streams, float* y, int32_t* path, float* carry, int32_t* state,
                                    const float* window, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  hipLaunchKernelGGL(timescale_stream_k, dim3((unsigned)n_streams), dim3(256), 0, st, x, tab, y, path, carry, state, window);
  return hipGetLastError();
}

hipError_t launch_time_scale_ragged(const float* x, const long long* off_in, float* y, const long long* off_out, int32_t* path,
                                    const long long* path_off, int n_seg, long long n_out_max, const float* window, int num, int den,
                                    hipStream_t st) {
  if (n_seg <= 0 || n_out_max <= 0) return hipSuccess;
  hipLaunchKernelGGL(timescale_path_k, dim3((unsigned)n_seg), dim3(256), 0, st, x, off_in, off_out, path, path_off, num, den);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((n_out_max + TS_TILE - 1) / TS_TILE), (unsigned)n_seg);
  hipLaunchKernelGGL(timescale_ola_k, grid, dim3(256), 0, st, x, off_in, y, off_out, path, path_off, window);
  return hipGetLastError();
}
