// IMA/DVI ADPCM on the device (ctts_adpcm_encode_ranges): 16-bit mono PCM -> the 4-bit blocks of a WAVE_FORMAT_IMA_ADPCM file, strictly
// behind the PCM16 conversion (codec.hip).  chattts_amd/adpcm.py is the NumPy twin, byte for byte, and states the definition: a block of
// `align` = 256 * max(1, rate / 11025) bytes holds S = 2 * (align - 4) + 1 samples -- its first sample and its start index in a 4-byte
// header, then one 4-bit code per sample, the earlier sample of a byte in the low bits.  The start index is a function of the block's
// first difference, so a block's bytes depend on its own samples only: every block of every range is independent work, and a block is
// S - 1 dependent steps.  Hence ONE LANE PER BLOCK.
// Table-driven: range r (AdpcmRange) says that elements [start, start + n) of the int16 input are one signal at `rate`; with
// count_idx >= 0 its length m is min(counts[count_idx], n), read on the device (float_to_int16_groups' kept counts).  The range owns
// the blocks [block0, block0 + ceil(n / S)) of the call and the bytes from byte0 on; it writes ceil(m / S) of them, positions at or
// beyond m reading as x[m - 1], and m itself to used[r].  One launch for all ranges: the blocks of the call are numbered through, lane g
// finds its range by bisection over block0, and a workgroup is one wave of 64 consecutive blocks -- neighbours in memory, also across a
// range's end.
// A lane must not stride through global memory S samples from its neighbour, so the block is cut into time tiles of 64 output bytes
// (128 samples; the first: the header and 120).  Per tile the wave stages the 16-byte units that cover each lane's window into LDS
// (consecutive threads take consecutive units of one block: 272 contiguous bytes; a unit that is not wholly the range's goes element by
// element), every lane steps through its window and leaves 16 words in LDS, and the wave stores each block's 64 bytes as four 16-byte
// units (byte0 is a multiple of 256: always aligned, always wholly the block's).  Row strides in LDS are odd numbers of words.  The
// step table lives in LDS (a lane's index is its own); the step itself is compares and selects.  Nothing outside a range's written
// blocks is written.  Plain vector stores only.  Positions are 64-bit.
// Streams (ctts_adpcm_stream_step, the end of this file): adpcm_stage_k in front of the same adpcm_encode_k, which then runs over the
// staging ranges and takes each range's length from the count that adpcm_stage_k wrote.
#include "common.hpp"
#include "kernels.hpp"

#define ADPCM_TILE 64                    // output bytes of one block per time tile
#define ADPCM_UNITS 17                   // 16-byte units that cover 128 samples at any alignment
#define ADPCM_XW (4 * ADPCM_UNITS + 1)   // a lane's window in LDS, in words
#define ADPCM_OW (ADPCM_TILE / 4 + 1)    // a lane's codes in LDS, in words

typedef uint32_t adpcm_u32x4 __attribute__((ext_vector_type(4)));

__constant__ int adpcm_step_c[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552,
    1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487,
    12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

__device__ __forceinline__ int adpcm_align(int rate) { return 256 * max(1, rate / 11025); }

// the signal length of a range as the device sees it
__device__ __forceinline__ long long adpcm_range_len(const AdpcmRange& R, const long long* __restrict__ counts) {
  if (R.rate <= 0) return 0;
  if (R.count_idx < 0) return R.n;
  const long long c = counts[R.count_idx];
  return c < 0 ? 0 : (c < R.n ? c : R.n);
}

// the first sample of tile k within its block, and the samples the tile consumes
__device__ __forceinline__ int adpcm_tile_first(int k) { return k ? 2 * ADPCM_TILE * k - 7 : 0; }
__device__ __forceinline__ int adpcm_tile_count(int k) { return k ? 2 * ADPCM_TILE : 2 * ADPCM_TILE - 7; }

__global__ __launch_bounds__(ADPCM_LANES) void adpcm_encode_k(const int16_t* __restrict__ pcm, const long long* __restrict__ counts,
                                                              const AdpcmRange* __restrict__ rng, int n_rng, long long n_blocks,
                                                              uint8_t* __restrict__ out, long long* __restrict__ used) {
  __shared__ uint32_t s_x[ADPCM_LANES * ADPCM_XW];
  __shared__ uint32_t s_o[ADPCM_LANES * ADPCM_OW];
  __shared__ int s_step[89];
  __shared__ long long s_e0[ADPCM_LANES], s_end[ADPCM_LANES], s_dst[ADPCM_LANES];   // a lane's first element (< 0: no block), its range's end, its first byte
  __shared__ int s_nt[ADPCM_LANES], s_nt_max;
  const int t = threadIdx.x;
  for (int i = t; i < 89; i += ADPCM_LANES) s_step[i] = adpcm_step_c[i];
  if (t == 0) s_nt_max = 0;
  if (blockIdx.x == 0)
    for (int r = t; r < n_rng; r += ADPCM_LANES) used[r] = adpcm_range_len(rng[r], counts);
  __syncthreads();

  const long long g = (long long)blockIdx.x * ADPCM_LANES + t;
  long long e0 = -1, end = 0, dst = 0;
  int nt = 0, left = 0, last = 0;        // tiles of the block; samples of the signal from the block's first on (up to S); x[m - 1]
  if (g < n_blocks) {
    int lo = 0, hi = n_rng - 1;          // the last range with block0 <= g owns block g (ranges without blocks share their successor's block0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (rng[mid].block0 <= g) lo = mid;
      else hi = mid - 1;
    }
    const AdpcmRange R = rng[lo];
    const long long m = adpcm_range_len(R, counts);
    const int A = adpcm_align(R.rate), S = 2 * (A - 4) + 1;
    const long long b = g - R.block0;
    if (b * S < m) {
      e0 = R.start + b * S;
      end = R.start + R.n;
      dst = R.byte0 + b * A;
      nt = A / ADPCM_TILE;
      left = (int)min(m - b * S, (long long)S);
      last = (int)pcm[R.start + m - 1];
    }
  }
  s_e0[t] = e0;
  s_end[t] = end;
  s_dst[t] = dst;
  s_nt[t] = nt;
  if (nt) atomicMax(&s_nt_max, nt);
  __syncthreads();
  const int nt_max = s_nt_max;

  int pred = 0, idx = 0;
  for (int k = 0; k < nt_max; ++k) {
    const int first = adpcm_tile_first(k), cnt = adpcm_tile_count(k);
    for (int it = t; it < ADPCM_LANES * ADPCM_UNITS; it += ADPCM_LANES) {
      const int row = it / ADPCM_UNITS, u = it - row * ADPCM_UNITS;
      const long long re = s_e0[row];
      if (re < 0 || k >= s_nt[row]) continue;
      const long long a0 = re + first, pos = ((a0 >> 3) + u) << 3;     // the window's first element; this unit's
      if (pos >= a0 + cnt) continue;
      uint32_t w[4];
      if (pos + 8 <= s_end[row]) {       // pcm is 16-byte aligned, pos a multiple of 8 elements
        const adpcm_u32x4 v = *reinterpret_cast<const adpcm_u32x4*>(pcm + pos);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      } else {                           // the unit is not wholly the range's
        const long long re_end = s_end[row];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t a = pos + 2 * j < re_end ? (uint32_t)(uint16_t)pcm[pos + 2 * j] : 0u;
          const uint32_t b = pos + 2 * j + 1 < re_end ? (uint32_t)(uint16_t)pcm[pos + 2 * j + 1] : 0u;
          w[j] = a | (b << 16);
        }
      }
      uint32_t* d = s_x + row * ADPCM_XW + 4 * u;
      d[0] = w[0]; d[1] = w[1]; d[2] = w[2]; d[3] = w[3];
    }
    __syncthreads();

    if (k < nt) {
      const int16_t* xs = reinterpret_cast<const int16_t*>(s_x + t * ADPCM_XW) + (int)((e0 + first) & 7);
      uint32_t* o = s_o + t * ADPCM_OW;
      int j = 0, w0 = 0;
      if (k == 0) {                      // the header: the first sample, and the least index whose step reaches the first difference
        pred = (int)xs[0];
        const int x1 = 1 < left ? (int)xs[1] : last;
        const int d = abs(x1 - pred);
        int i0 = 0;
#pragma unroll
        for (int bit = 64; bit; bit >>= 1) {
          const int c = i0 + bit;
          i0 = (c <= 88 && s_step[min(c, 89) - 1] < d) ? c : i0;
        }
        idx = i0;
        o[0] = ((uint32_t)pred & 0xFFFFu) | ((uint32_t)idx << 16);
        j = 1;
        w0 = 1;
      }
      for (int w = w0; w < ADPCM_TILE / 4; ++w) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q, ++j) {
          const int v = first + j < left ? (int)xs[j] : last;
          const int step = s_step[idx];
          int d = v - pred;
          const int neg = d < 0;
          d = abs(d);
          int vp = step >> 3;
          const int c4 = d >= step;
          d -= c4 ? step : 0;
          vp += c4 ? step : 0;
          const int c2 = d >= (step >> 1);
          d -= c2 ? (step >> 1) : 0;
          vp += c2 ? (step >> 1) : 0;
          const int c1 = d >= (step >> 2);
          vp += c1 ? (step >> 2) : 0;
          const int mag = (c4 << 2) | (c2 << 1) | c1;
          pred = min(max(pred + (neg ? -vp : vp), -32768), 32767);
          idx = min(max(idx + (mag < 4 ? -1 : 2 * (mag - 3)), 0), 88);      // IDX = -1 -1 -1 -1 2 4 6 8
          word |= (uint32_t)(mag | (neg << 3)) << (4 * q);
        }
        o[w] = word;
      }
    }
    __syncthreads();

    for (int it = t; it < ADPCM_LANES * (ADPCM_TILE / 16); it += ADPCM_LANES) {
      const int row = it / (ADPCM_TILE / 16), u = it % (ADPCM_TILE / 16);
      if (s_e0[row] < 0 || k >= s_nt[row]) continue;
      const uint32_t* o = s_o + row * ADPCM_OW + 4 * u;
      adpcm_u32x4 v;
      v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
      *reinterpret_cast<adpcm_u32x4*>(out + s_dst[row] + (long long)k * ADPCM_TILE + 16 * u) = v;
    }
  }
}

hipError_t launch_adpcm_encode(const int16_t* pcm, const long long* counts, const AdpcmRange* rng, int n_rng, long long n_blocks, uint8_t* out,
                               long long* used, hipStream_t st) {
  if (n_rng <= 0 || n_blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(adpcm_encode_k, dim3((unsigned)((n_blocks + ADPCM_LANES - 1) / ADPCM_LANES)), dim3(ADPCM_LANES), 0, st, pcm, counts, rng,
                     n_rng, n_blocks, out, used);
  return hipGetLastError();
}

// ---- streams (ctts_adpcm_stream_step) ----------------------------------------------------------------------------------------------
// One workgroup per push: [the stream's carried samples | the push's samples, a final push's shortened by its count and compacted by
// its keep mask] go to the push's 16-byte-aligned staging range, so that adpcm_encode_k's aligned path serves the blocks cut from it.
// The cutting rule of chattts_amd/adpcm.py (stream_plan): whole blocks of S samples leave from the front, the rest waits in the
// stream's slot (state [slots][ADPCM_CARRY] int16) unless the push is final, which emits everything and holds nothing.  The slot is
// read into LDS before the barrier and written behind it, by this workgroup alone (the host refuses a slot named twice).  A keep mask
// is MSB first and starts at byte start / 8.  Thread 0 writes what adpcm_encode_k reads: the push's AdpcmRange over its staging range
// (its length the count written here: `emit` for a push that is not final, what is held for a final one), and the same count to used.
__global__ __launch_bounds__(1024) void adpcm_stage_k(const int16_t* __restrict__ pcm, const uint8_t* __restrict__ mask,
                                                      const long long* __restrict__ counts, const AdpcmPush* __restrict__ push,
                                                      int16_t* __restrict__ state, int16_t* __restrict__ stage, AdpcmRange* __restrict__ rng,
                                                      long long* __restrict__ staged, long long* __restrict__ used) {
  __shared__ int16_t s_c[ADPCM_CARRY];
  __shared__ int s_v[2][1024];
  __shared__ long long s_run;
  const AdpcmPush P = push[blockIdx.x];
  const int t = threadIdx.x;
  const int c = P.carry;
  const bool last = P.flags & 1, masked = P.flags & 2;
  int16_t* slot = state + (long long)P.slot * ADPCM_CARRY;
  for (int i = t; i < c; i += 1024) s_c[i] = slot[i];
  if (t == 0) s_run = 0;
  long long L = P.n;
  if (P.count_idx >= 0) {
    const long long k = counts[P.count_idx];
    L = k < 0 ? 0 : (k < L ? k : L);
  }
  __syncthreads();
  // a push that is not final has neither a count nor a mask: what it holds and emits is known before a sample is read
  const long long S = 2 * (adpcm_align(P.rate) - 4) + 1;
  const long long emit = last ? (1ll << 62) : (c + L) / S * S;
  int16_t* dst = stage + P.stage;
  const int16_t* src = pcm + P.start;
  for (int i = t; i < c; i += 1024) {
    dst[i] = s_c[i];
    if (i >= emit) slot[i - emit] = s_c[i];
  }
  for (long long tile = 0; tile < L; tile += 8 * 1024) {
    const long long i0 = tile + 8 * t;
    uint32_t bits = 0;
    if (i0 < L) {
      bits = masked ? mask[(P.start + i0) >> 3] : 0xFFu;
      if (L - i0 < 8) bits &= (0xFFu << (8 - (int)(L - i0))) & 0xFFu;
    }
    const int cnt = __popc(bits);
    long long pos = i0;
    if (masked) {
      int cur = 0;
      s_v[0][t] = cnt;
      __syncthreads();
      for (int d = 1; d < 1024; d <<= 1) {
        s_v[cur ^ 1][t] = s_v[cur][t] + (t >= d ? s_v[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
      }
      const long long run = s_run;
      pos = run + s_v[cur][t] - cnt;
      __syncthreads();
      if (t == 1023) s_run = run + s_v[cur][t];
    }
    if (bits) {
      int16_t x[8];
      if (i0 + 8 <= L) {                 // pcm is 16-byte aligned and starts are multiples of 8 elements
        const int4 a = *reinterpret_cast<const int4*>(src + i0);
        const int w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          x[2 * j] = (int16_t)(w[j] & 0xFFFF);
          x[2 * j + 1] = (int16_t)(w[j] >> 16);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = i0 + j < L ? src[i0 + j] : (int16_t)0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (bits & (0x80u >> j)) {
          const long long d = c + pos++;
          dst[d] = x[j];
          if (d >= emit) slot[d - emit] = x[j];
        }
    }
  }
  __syncthreads();
  if (t == 0) {
    const long long held = c + (masked ? s_run : L);
    AdpcmRange R;
    R.start = P.stage;
    R.n = last ? c + P.n : emit;
    R.block0 = P.block0;
    R.byte0 = P.byte0;
    R.rate = P.rate;
    R.count_idx = (int32_t)blockIdx.x;
    R.reserved = 0;
    rng[blockIdx.x] = R;
    staged[blockIdx.x] = used[blockIdx.x] = last ? held : emit;
  }
}

hipError_t launch_adpcm_stream(const int16_t* pcm, const uint8_t* mask, const long long* counts, const AdpcmPush* push, int n_push,
                               int16_t* state, long long n_blocks, uint8_t* out, long long* used, long long* staged, AdpcmRange* rng,
                               int16_t* stage, hipStream_t st) {
  if (n_push <= 0) return hipSuccess;
  hipLaunchKernelGGL(adpcm_stage_k, dim3((unsigned)n_push), dim3(1024), 0, st, pcm, mask, counts, push, state, stage, rng, staged, used);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_adpcm_encode((const int16_t*)stage, (const long long*)staged, (const AdpcmRange*)rng, n_push, n_blocks, out, used, st);
}
