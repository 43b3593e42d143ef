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

// A STREAM (ctts_resample_stream_step, ctts_codec_decode_windows_speed_rate): the signal arrives in pushes and exists nowhere as a whole -- the
// time scaler's stream, say -- so the history and the look-ahead of the filter are carried.  With `pos` samples pushed before and n_in
// arriving, the step emits outputs [o_lo, o_lo + n_out) of the signal's conversion (resample.py, stream_plan: every output whose inputs
// [j M - width, j M + width + M) have arrived; on the last push, total = pos + n_in, all that remain).  A read at signal position g comes from
// the new samples x[in_off + g - pos] (g >= pos), from the slot's carry, which holds samples [pos - c_in, pos), or is zero (g < 0, or
// g >= total on the last push: the segment-alone rule).  The host guarantees that nothing below pos - c_in is read.  Tiles, staging and
// accumulation are resample_win_k's, hence the chunks of a stream, concatenated, equal resample_seg_k over the whole signal bit for bit,
// however the signal was cut.  The descriptor's FIRST workgroup also writes the next carry, samples [pos + n_in - c_out, pos + n_in), into
// the slot's OTHER buffer (carry [slots][2][RS_CARRY]: a step reads buffer `phase` and writes the other, so the workgroups that still read
// the old carry in this launch never meet the write: no atomics, no waiting); it runs when the step emits nothing, too.
__device__ __forceinline__ float rs_stream_read(const float* __restrict__ xin, const float* __restrict__ cold, long long g, long long c,
                                                long long pos, long long end) {
  if (g >= pos) return g < end ? xin[g - pos] : 0.0f;
  return g >= c ? cold[g - c] : 0.0f;            // g < c only where g < 0
}

template <bool TAB_LDS>
__global__ __launch_bounds__(256) void resample_stream_k(const float* __restrict__ x, const RsStream* __restrict__ tab, float* __restrict__ y,
                                                         float* __restrict__ carry, const float* __restrict__ taps, int L, int M, int K) {
  extern __shared__ __align__(16) float rs_lds[];
  const RsStream& W = tab[blockIdx.y];
  const long long n_out = W.n_out;
  const long long r0 = (long long)blockIdx.x * RS_TILE;      // the tile's first output, relative to the chunk
  const bool has = r0 < n_out;
  if (!has && blockIdx.x != 0) return;           // the whole workgroup: nothing waits at a barrier
  const long long pos = W.pos, end = pos + W.n_in, c = pos - W.c_in;
  const float* xin = x + W.in_off;
  const float* cold = carry + ((long long)W.slot * 2 + W.phase) * RS_CARRY;
  if (has) {                                     // workgroup-uniform
    const long long o0 = W.o_lo + r0;
    const int m = (int)min((long long)RS_TILE, n_out - r0);
    const int width = (K - M) >> 1;
    const long long j0 = o0 / L, j1 = (o0 + m - 1) / L;
    const int span = (int)(j1 - j0) * M + K;     // <= rs_span_max(L, M, K) for any phase of o0
    const long long in0 = j0 * (long long)M - width;   // the tile's first input sample, in the signal
    float* hs = rs_lds;
    float* xs = rs_lds + (TAB_LDS ? L * K : 0);
    if (TAB_LDS)
      for (int e = threadIdx.x; e < L * K; e += 256) hs[(e % K) * L + e / K] = taps[e];
    for (int e = threadIdx.x; e < span; e += 256) xs[e] = rs_stream_read(xin, cold, in0 + e, c, pos, end);
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
  if (blockIdx.x == 0 && W.total < 0) {          // more to come: keep samples [end - c_out, end); c_out <= RS_CARRY, the host refused the rest
    float* cnew = carry + ((long long)W.slot * 2 + (W.phase ^ 1)) * RS_CARRY;
    const long long nb = end - W.c_out;          // >= c: a carry never reaches back beyond the one before it
    for (int i = threadIdx.x; i < W.c_out; i += 256) cnew[i] = rs_stream_read(xin, cold, nb + i, c, pos, end);
  }
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

hipError_t launch_resample_stream(const float* x, const RsStream* tab, int n_streams, long long n_out_max, float* y, float* carry,
                                  const float* taps, int L, int M, int K, hipStream_t st) {
  const int mode = resample_mode(L, M, K);
  if (mode == 0) return hipErrorInvalidValue;
  if (n_streams <= 0) return hipSuccess;
  // at least one workgroup per descriptor: a step that emits nothing still appends its push to the carry
  const long long tiles = (n_out_max + RS_TILE - 1) / RS_TILE;
  const dim3 grid((unsigned)(tiles > 0 ? tiles : 1), (unsigned)n_streams);
  const size_t lds = sizeof(float) * (size_t)(rs_span_max(L, M, K) + (mode == 2 ? (long long)L * K : 0));
  if (mode == 2) hipLaunchKernelGGL(resample_stream_k<true>, grid, dim3(256), lds, st, x, tab, y, carry, taps, L, M, K);
  else hipLaunchKernelGGL(resample_stream_k<false>, grid, dim3(256), lds, st, x, tab, y, carry, taps, L, M, K);
  return hipGetLastError();
}
