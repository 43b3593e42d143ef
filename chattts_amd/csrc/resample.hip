// Sample-rate conversion on the device (ctts_resample_ragged): rational polyphase resampling by L/M over packed segments, the layout the
// ragged decoder writes (samples [off[s], off[s+1]) are segment s).  Every segment is converted as if alone: input positions outside its
// own [0, n_s) read as zero, like the ragged convolutions' loaders mask.
//   y[j L + i] = sum_k h[i][k] x[j M + k - width],   k = 0 .. K-1,  width = (K - M) / 2,  h: [L][K] float32 (chattts_amd/resample.py)
// One accumulator per output sample, k ascending, fmaf: a sample's bits depend on its own segment's samples alone -- not on what it is
// packed with, nor on where the tiles fall.
// A workgroup converts a tile of RS_TILE consecutive output samples of one segment.  It stages the input span those outputs read
// ((j1 - j0) M + K samples, masked at the segment's edges) in LDS with coalesced loads, and -- where both fit RS_LDS_FLOATS -- the filter
// table too, transposed to [K][L] so that lanes on consecutive outputs (consecutive phases i) read consecutive LDS words; a larger table
// is read through L2.  Thread t owns outputs t, t + 256, ...: coalesced stores.  Positions (j M, the segment offsets) are 64-bit; within
// a tile everything is relative to the tile's first input sample and fits an int.
#include "common.hpp"
#include "kernels.hpp"

template <bool TAB_LDS>
__global__ __launch_bounds__(256) void resample_seg_k(const float* __restrict__ x, const long long* __restrict__ off_in, float* __restrict__ y,
                                                      const long long* __restrict__ off_out, const int32_t* __restrict__ sel,
                                                      const float* __restrict__ taps, int L, int M, int K) {
  extern __shared__ __align__(16) float rs_lds[];
  const int s = sel != nullptr ? sel[blockIdx.y] : (int)blockIdx.y;
  const long long lo = off_in[s], n_in = off_in[s + 1] - lo;
  const long long olo = off_out[s], n_out = off_out[s + 1] - olo;
  const long long o0 = (long long)blockIdx.x * RS_TILE;
  if (o0 >= n_out) return;                       // the whole workgroup: nothing waits at a barrier
  const int m = (int)min((long long)RS_TILE, n_out - o0);
  const int width = (K - M) >> 1;
  const long long j0 = o0 / L, j1 = (o0 + m - 1) / L;
  const int span = (int)(j1 - j0) * M + K;       // <= rs_span_max(L, M, K): the host sized the LDS for it
  const long long in0 = j0 * (long long)M - width;   // the tile's first input sample, relative to the segment
  float* hs = rs_lds;
  float* xs = rs_lds + (TAB_LDS ? L * K : 0);
  if (TAB_LDS)
    for (int e = threadIdx.x; e < L * K; e += 256) hs[(e % K) * L + e / K] = taps[e];
  for (int e = threadIdx.x; e < span; e += 256) {
    const long long g = in0 + e;
    xs[e] = (g >= 0 && g < n_in) ? x[lo + g] : 0.0f;
  }
  __syncthreads();
  const unsigned i0 = (unsigned)(o0 - j0 * L);   // phase of the tile's first output, < L
  for (int t = threadIdx.x; t < m; t += 256) {
    const unsigned q = i0 + (unsigned)t;
    const int dj = (int)(q / (unsigned)L), i = (int)(q % (unsigned)L);
    const float* xp = xs + dj * M;
    float acc = 0.0f;
    if (TAB_LDS) {
      for (int k = 0; k < K; ++k) acc = fmaf(hs[k * L + i], xp[k], acc);
    } else {
      const float* hp = taps + (size_t)i * K;
      for (int k = 0; k < K; ++k) acc = fmaf(hp[k], xp[k], acc);
    }
    y[olo + o0 + t] = acc;
  }
}

// A WINDOW of a longer signal, at an arbitrary output phase (ctts_resample_windows, ctts_codec_decode_windows_rate): the window holds samples
// [origin, origin + n_in) of the signal and outputs [o_lo, o_hi) of the signal's conversion are wanted -- a streamed chunk.  A workgroup
// converts RS_TILE consecutive outputs from o_lo + blockIdx.x RS_TILE on (not a multiple of the tile in signal coordinates); the staged span
// starts at input (o_tile / L) M - width of the signal, i.e. that minus `origin` of the window, and positions outside the window's samples
// read as zero.  The host guarantees that every input the outputs read inside the signal's [0, total) lies in the window (capi.hip checks
// it against resample.py's window_inputs), so the zeros stand only for samples outside the signal: the segment-alone rule.  The accumulation
// is resample_seg_k's (one accumulator, k ascending, fmaf; fmaf(h, 0, acc) adds nothing), hence a chunk equals outputs [o_lo, o_hi) of
// resample_seg_k over the whole signal bit for bit, wherever the tiles fall.  The `pad` elements behind the chunk are written as zeros.
template <bool TAB_LDS>
__global__ __launch_bounds__(256) void resample_win_k(const float* __restrict__ x, const RsWindow* __restrict__ win, float* __restrict__ y,
                                                      const int32_t* __restrict__ sel, const float* __restrict__ taps, int L, int M, int K) {
  extern __shared__ __align__(16) float rs_lds[];
  const RsWindow& W = win[sel != nullptr ? sel[blockIdx.y] : (int)blockIdx.y];
  const long long n_in = W.n_in, n_out = W.o_hi - W.o_lo;
  const long long r0 = (long long)blockIdx.x * RS_TILE;      // the tile's first output, relative to the chunk
  if (r0 >= n_out) return;                       // the whole workgroup: nothing waits at a barrier
  const long long o0 = W.o_lo + r0;
  const int m = (int)min((long long)RS_TILE, n_out - r0);
  const int width = (K - M) >> 1;
  const long long j0 = o0 / L, j1 = (o0 + m - 1) / L;
  const int span = (int)(j1 - j0) * M + K;       // <= rs_span_max(L, M, K) for any phase of o0
  const long long in0 = j0 * (long long)M - width - W.origin;   // the tile's first input sample, relative to the window
  float* hs = rs_lds;
  float* xs = rs_lds + (TAB_LDS ? L * K : 0);
  if (TAB_LDS)
    for (int e = threadIdx.x; e < L * K; e += 256) hs[(e % K) * L + e / K] = taps[e];
  const float* xw = x + W.in_off;
  for (int e = threadIdx.x; e < span; e += 256) {
    const long long g = in0 + e;
    xs[e] = (g >= 0 && g < n_in) ? xw[g] : 0.0f;
  }
  __syncthreads();
  float* yw = y + W.out_off + r0;
  const unsigned i0 = (unsigned)(o0 - j0 * L);   // phase of the tile's first output, < L
  for (int t = threadIdx.x; t < m; t += 256) {
    const unsigned q = i0 + (unsigned)t;
    const int dj = (int)(q / (unsigned)L), i = (int)(q % (unsigned)L);
    const float* xp = xs + dj * M;
    float acc = 0.0f;
    if (TAB_LDS) {
      for (int k = 0; k < K; ++k) acc = fmaf(hs[k * L + i], xp[k], acc);
    } else {
      const float* hp = taps + (size_t)i * K;
      for (int k = 0; k < K; ++k) acc = fmaf(hp[k], xp[k], acc);
    }
    yw[t] = acc;
  }
  if (r0 + m == n_out && (int)threadIdx.x < W.pad) yw[m + threadIdx.x] = 0.0f;   // the chunk's last tile: the zero pad
}

// the longest input span of a tile, in samples: outputs o0 .. o0 + RS_TILE - 1 touch at most (RS_TILE - 1) / L + 2 input frames j
long long rs_span_max(int L, int M, int K) { return ((long long)(RS_TILE - 1) / L + 1) * M + K; }

// 0: the pair is not supported (the span does not fit the LDS, or the table is beyond RS_TAB_MAX floats); 1: table through L2; 2: table in LDS
int resample_mode(int L, int M, int K) {
  if (L < 1 || M < 1 || L == M || K <= M || ((K - M) & 1)) return 0;
  const long long span = rs_span_max(L, M, K), tab = (long long)L * K;
  if (span > RS_LDS_FLOATS || tab > RS_TAB_MAX) return 0;
  return tab + span <= RS_LDS_FLOATS ? 2 : 1;
}

hipError_t launch_resample_ragged(const float* x, const long long* off_in, float* y, const long long* off_out, const int32_t* sel, int n_launch,
                                  long long n_out_max, const float* taps, int L, int M, int K, hipStream_t st) {
  const int mode = resample_mode(L, M, K);
  if (mode == 0) return hipErrorInvalidValue;
  if (n_launch <= 0 || n_out_max <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_out_max + RS_TILE - 1) / RS_TILE), (unsigned)n_launch);
  const size_t lds = sizeof(float) * (size_t)(rs_span_max(L, M, K) + (mode == 2 ? (long long)L * K : 0));
  if (mode == 2) hipLaunchKernelGGL(resample_seg_k<true>, grid, dim3(256), lds, st, x, off_in, y, off_out, sel, taps, L, M, K);
  else hipLaunchKernelGGL(resample_seg_k<false>, grid, dim3(256), lds, st, x, off_in, y, off_out, sel, taps, L, M, K);
  return hipGetLastError();
}

hipError_t launch_resample_windows(const float* x, const RsWindow* win, float* y, const int32_t* sel, int n_launch, long long n_out_max,
                                   const float* taps, int L, int M, int K, hipStream_t st) {
  const int mode = resample_mode(L, M, K);
  if (mode == 0) return hipErrorInvalidValue;
  if (n_launch <= 0 || n_out_max <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_out_max + RS_TILE - 1) / RS_TILE), (unsigned)n_launch);
  const size_t lds = sizeof(float) * (size_t)(rs_span_max(L, M, K) + (mode == 2 ? (long long)L * K : 0));
  if (mode == 2) hipLaunchKernelGGL(resample_win_k<true>, grid, dim3(256), lds, st, x, win, y, sel, taps, L, M, K);
  else hipLaunchKernelGGL(resample_win_k<false>, grid, dim3(256), lds, st, x, win, y, sel, taps, L, M, K);
  return hipGetLastError();
}
