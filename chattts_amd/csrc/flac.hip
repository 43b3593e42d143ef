// FLAC on the device (ctts_flac_encode_ranges): 16-bit mono PCM -> FLAC frames, strictly behind the PCM16 conversion (codec.hip).  The subset
// is fixed so that chattts_amd/flac.py, the NumPy twin, agrees byte for byte: fixed block size 4096 (a shorter last block carries n - 1 in
// 16 bits), the rate by its table code or in Hz, one subframe per frame -- CONSTANT when all samples are equal, else FIXED order o in
// 0 .. min(4, n - 1) with Rice partition order p in 0 .. min(6, ctz(n)), (n >> p) > o, parameters k in 0 .. 14, when STRICTLY smaller than
// VERBATIM.  The choice is an exact search: the smallest subframe in bits over every (o, p, k per partition), ties to the lowest o, then
// the lowest p, then the lowest k.  All sums are 64-bit (order-4 residuals reach 20 bits; 4096 of them pass 2^32).
// Table-driven: range r (FlacRange) says that elements [start, start + n) of the int16 input are one signal at `rate`; with count_idx >= 0
// its length is min(counts[count_idx], n), read on the device (float_to_int16_groups' kept counts).  Range r owns the frame slots
// [frame0, frame0 + ceil(n / 4096)).  Three launches whatever the number of ranges:
//   1. flac_analyse_k, one workgroup per slot: the five residuals of each sample, the 15 Rice sums per finest partition (a thread owns 16
//      consecutive samples, sums in registers, and flushes with 64-bit LDS adds when the partition changes), the sums folded up the
//      partition orders, the exact choice; the frame's length in bytes and its parameters go to the slot's FlacFrame (length 0: no frame).
//   2. flac_scan_k, one workgroup: the exclusive byte offsets of all slots in order, so that the frames of the call lie back to back
//      and a range's frames form one slice; off[n_frames] is the total.
//   3. flac_pack_k, one workgroup per frame: the header with its CRC-8, a scan of the per-sample code lengths, the bits OR-ed big-endian
//      into zeroed LDS (a code's unary run costs nothing; the stop bit and the k low bits are at most 15 bits: two words), the CRC-16 from
//      per-thread pieces (CRC with initial value 0 is linear: piece t is advanced by x^(8 * bytes behind it) mod the polynomial), then
//      16-byte stores to the final position (bytes where a 16-byte unit of the destination is not wholly the frame's).
// Bytes of `out` outside [0, off[n_frames]) are not written.  Plain vector stores and LDS atomics only.
// Streams (ctts_flac_stream_step, the end of this file): flac_stage_k in front of the same three kernels, which then take the number of
// each range's first sample (`base`) and write variable-block-size frames (FF F9) numbered by their first sample, in up to 36 bits.
#include "common.hpp"
#include "kernels.hpp"

#define FLAC_MAX_ORDER 4
#define FLAC_MAX_PART 6
#define FLAC_RICE 15                     // parameters 0 .. 14
// a frame is at most 19 + 2 * 4096 bytes (a stream's header: up to 16 bytes, never all of them at 4096 samples); the store loop's
// unaligned reads and the CRC's second word reach one word further: 2053 words at the most
#define FLAC_WORDS (FLAC_BLOCK / 2 + 8)

typedef uint32_t flac_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long flac_u64;

__device__ __forceinline__ int flac_rate_code(int rate) {
  switch (rate) {
    case 88200: return 1;
    case 176400: return 2;
    case 192000: return 3;
    case 8000: return 4;
    case 16000: return 5;
    case 22050: return 6;
    case 24000: return 7;
    case 32000: return 8;
    case 44100: return 9;
    case 48000: return 10;
    case 96000: return 11;
  }
  return 13;                             // Hz in 16 bits (the host refused every rate that fits neither form)
}

// the UTF-8-like coding of a frame's number: the frame's index (fixed block size), or its first sample's number in up to 36 bits (a stream)
__device__ __forceinline__ int flac_number_bytes(flac_u64 f) {
  return f < 0x80ull ? 1 : f < 0x800ull ? 2 : f < 0x10000ull ? 3 : f < 0x200000ull ? 4 : f < 0x4000000ull ? 5 : f < 0x80000000ull ? 6 : 7;
}

// the number frame slot f of range r carries: f itself, or in a stream (base given) the number of its first sample, base[r] + 4096 f
__device__ __forceinline__ flac_u64 flac_frame_number(const long long* __restrict__ base, int r, long long f) {
  return base ? (flac_u64)(base[r] + f * (long long)FLAC_BLOCK) : (flac_u64)f;
}

__device__ __forceinline__ uint32_t flac_zigzag(int r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// the signal length of a range as the device sees it
__device__ __forceinline__ long long flac_range_len(const FlacRange& R, const long long* __restrict__ counts) {
  if (R.rate <= 0) return 0;
  if (R.count_idx < 0) return R.n;
  const long long c = counts[R.count_idx];
  return c < 0 ? 0 : (c < R.n ? c : R.n);
}

// block samples [0, n) of the frame into LDS, as int32 behind four zeros (the predictors read up to four samples back)
__device__ __forceinline__ void flac_load_block(const int16_t* __restrict__ src, int n, int* __restrict__ s_x) {
  const int t = threadIdx.x;
  if (t < 4) s_x[t] = 0;
  const int i0 = t * 16;
  if (i0 + 16 <= n) {                    // src is 16-byte aligned: starts are multiples of 8 elements, blocks of 4096
    const int4 a = *reinterpret_cast<const int4*>(src + i0);
    const int4 b = *reinterpret_cast<const int4*>(src + i0 + 8);
    const int w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s_x[4 + i0 + 2 * j] = (int)(int16_t)(w[j] & 0xFFFF);
      s_x[4 + i0 + 2 * j + 1] = w[j] >> 16;
    }
  } else {
    for (int j = 0; j < 16; ++j) s_x[4 + i0 + j] = i0 + j < n ? (int)src[i0 + j] : 0;
  }
}

__global__ __launch_bounds__(256) void flac_analyse_k(const int16_t* __restrict__ pcm, const long long* __restrict__ counts,
                                                      const FlacRange* __restrict__ rng, FlacFrame* __restrict__ rec,
                                                      long long* __restrict__ n_act, const long long* __restrict__ base) {
  __shared__ int s_x[FLAC_BLOCK + 4];
  __shared__ flac_u64 s_sum[FLAC_MAX_ORDER + 1][FLAC_RICE][1 << FLAC_MAX_PART];
  __shared__ flac_u64 s_tot[FLAC_MAX_ORDER + 1][FLAC_MAX_PART + 1];
  __shared__ uint8_t s_k[FLAC_MAX_ORDER + 1][2 << FLAC_MAX_PART];   // level p's parameters from (1 << p) - 1 on
  __shared__ int s_differs, s_pick[2];
  const FlacRange R = rng[blockIdx.y];
  const int t = threadIdx.x;
  const long long len = flac_range_len(R, counts);
  if (blockIdx.x == 0 && t == 0) n_act[blockIdx.y] = len;
  const long long slots = R.rate <= 0 ? 0 : (R.n + FLAC_BLOCK - 1) / FLAC_BLOCK;
  const long long f = blockIdx.x;
  if (f >= slots) return;
  FlacFrame* fr = rec + R.frame0 + f;
  const long long left = len - f * FLAC_BLOCK;
  if (left <= 0) {
    if (t == 0) fr->len = 0;
    return;
  }
  const int n = left < FLAC_BLOCK ? (int)left : FLAC_BLOCK;
  flac_load_block(pcm + R.start + f * FLAC_BLOCK, n, s_x);
  for (int i = t; i < (FLAC_MAX_ORDER + 1) * FLAC_RICE * (1 << FLAC_MAX_PART); i += 256) (&s_sum[0][0][0])[i] = 0;
  if (t < (FLAC_MAX_ORDER + 1) * (FLAC_MAX_PART + 1)) (&s_tot[0][0])[t] = 0;
  if (t == 0) s_differs = 0;
  __syncthreads();

  const int P = min(FLAC_MAX_PART, __ffs(n) - 1);      // the finest partition order
  const int S = n >> P;                                // its partition size
  const int omax = min(FLAC_MAX_ORDER, n - 1);
  {
    uint32_t acc[FLAC_MAX_ORDER + 1][FLAC_RICE];
#pragma unroll
    for (int o = 0; o <= FLAC_MAX_ORDER; ++o)
#pragma unroll
      for (int k = 0; k < FLAC_RICE; ++k) acc[o][k] = 0;
    const int i0 = t * 16, i1 = min(i0 + 16, n);
    const int first = s_x[4];
    int differs = 0, part = i0 < n ? i0 / S : 0;
#pragma unroll 1
    for (int i = i0; i <= i1; ++i) {
      const int pi = i < i1 ? i / S : -1;
      if (pi != part) {                                // the partition ends here (or the thread's samples do): flush
#pragma unroll
        for (int o = 0; o <= FLAC_MAX_ORDER; ++o)
#pragma unroll
          for (int k = 0; k < FLAC_RICE; ++k) {
            if (acc[o][k]) atomicAdd(&s_sum[o][k][part], (flac_u64)acc[o][k]);
            acc[o][k] = 0;
          }
        part = pi;
      }
      if (i >= i1) break;
      const int a0 = s_x[4 + i], a1 = s_x[3 + i], a2 = s_x[2 + i], a3 = s_x[1 + i], a4 = s_x[i];
      differs |= a0 != first;
      uint32_t u[FLAC_MAX_ORDER + 1];
      u[0] = flac_zigzag(a0);
      u[1] = i >= 1 ? flac_zigzag(a0 - a1) : 0u;       // a warm-up sample has no residual: it adds nothing to the sums
      u[2] = i >= 2 ? flac_zigzag(a0 - 2 * a1 + a2) : 0u;
      u[3] = i >= 3 ? flac_zigzag(a0 - 3 * a1 + 3 * a2 - a3) : 0u;
      u[4] = i >= 4 ? flac_zigzag(a0 - 4 * a1 + 6 * a2 - 4 * a3 + a4) : 0u;
#pragma unroll
      for (int o = 0; o <= FLAC_MAX_ORDER; ++o)
#pragma unroll
        for (int k = 0; k < FLAC_RICE; ++k) acc[o][k] += u[o] >> k;
    }
    if (differs) atomicOr(&s_differs, 1);
  }
  __syncthreads();

  for (int p = P; p >= 0; --p) {
    const int np = 1 << p, size = n >> p;
    for (int item = t; item < (omax + 1) * np; item += 256) {
      const int o = item >> p, j = item & (np - 1);
      if (size <= o) continue;
      const flac_u64 cnt = (flac_u64)(size - (j == 0 ? o : 0));
      flac_u64 best = ~0ull;
      int bk = 0;
      for (int k = 0; k < FLAC_RICE; ++k) {
        const flac_u64 c = s_sum[o][k][j] + cnt * (flac_u64)(k + 1);
        if (c < best) { best = c; bk = k; }            // strict: the lowest k of a tie
      }
      s_k[o][np - 1 + j] = (uint8_t)bk;
      atomicAdd(&s_tot[o][p], best + 4);
    }
    __syncthreads();
    if (p > 0) {
      // fold level p into level p - 1 in place: one thread per (o, k) row, ascending j, reads [2j], [2j + 1] before it writes [j]
      if (t < (FLAC_MAX_ORDER + 1) * FLAC_RICE) {
        flac_u64* row = &s_sum[0][0][0] + t * (1 << FLAC_MAX_PART);
        for (int j = 0; j < np / 2; ++j) row[j] = row[2 * j] + row[2 * j + 1];
      }
      __syncthreads();
    }
  }

  if (t == 0) {
    flac_u64 best = 8ull + 16ull * (flac_u64)n;        // VERBATIM
    int kind = 1, bo = 0, bp = 0;
    for (int o = 0; o <= omax; ++o)
      for (int p = 0; p <= P; ++p) {
        if ((n >> p) <= o) break;
        const flac_u64 bits = 8ull + 16ull * o + 6ull + s_tot[o][p];
        if (bits < best) { best = bits; kind = 2; bo = o; bp = p; }
      }
    if (!s_differs) { kind = 0; best = 24; bo = 0; bp = 0; }
    const int hdr = 4 + flac_number_bytes(flac_frame_number(base, blockIdx.y, f)) + (n != FLAC_BLOCK ? 2 : 0) + (flac_rate_code(R.rate) == 13 ? 2 : 0) + 1;
    fr->kind = kind;
    fr->order = bo;
    fr->part = bp;
    fr->bits = (int)best;
    fr->n = n;
    fr->hdr = hdr;
    fr->number = (int)f;
    fr->len = hdr + (int)((best + 7) >> 3) + 2;
    s_pick[0] = bo;
    s_pick[1] = bp;
  }
  __syncthreads();
  if (t < (1 << FLAC_MAX_PART)) fr->k[t] = t < (1 << s_pick[1]) ? s_k[s_pick[0]][(1 << s_pick[1]) - 1 + t] : 0;
}

__global__ __launch_bounds__(1024) void flac_scan_k(const FlacFrame* __restrict__ rec, long long n_frames, long long* __restrict__ off) {
  __shared__ long long s_v[2][1024];
  __shared__ long long s_carry;
  const int t = threadIdx.x;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (long long base = 0; base < n_frames; base += 1024) {
    const long long v = base + t < n_frames ? (long long)rec[base + t].len : 0;
    int cur = 0;
    s_v[0][t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      s_v[cur ^ 1][t] = s_v[cur][t] + (t >= d ? s_v[cur][t - d] : 0);
      cur ^= 1;
      __syncthreads();
    }
    const long long carry = s_carry;
    if (base + t < n_frames) off[base + t] = carry + s_v[cur][t] - v;
    __syncthreads();
    if (t == 1023) s_carry = carry + s_v[cur][t];
    __syncthreads();
  }
  if (t == 0) off[n_frames] = s_carry;
}

// ORs the `width` (1 .. 16) low bits of v into the big-endian bit stream at bit `pos`
__device__ __forceinline__ void flac_put(uint32_t* __restrict__ s_w, uint32_t pos, uint32_t v, int width) {
  const flac_u64 x = (flac_u64)v << (64 - (int)(pos & 31u) - width);
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  if (hi) atomicOr(&s_w[pos >> 5], hi);
  if (lo) atomicOr(&s_w[(pos >> 5) + 1], lo);
}

__device__ __forceinline__ uint32_t flac_byte(const uint32_t* __restrict__ s_w, int b) { return (s_w[b >> 2] >> (24 - 8 * (b & 3))) & 0xFFu; }

__device__ __forceinline__ uint32_t flac_mulmod16(uint32_t a, uint32_t b) {   // a * b mod x^16 + x^15 + x^2 + 1 over GF(2)
  uint32_t r = 0;
#pragma unroll
  for (int i = 15; i >= 0; --i) {
    r = (r << 1) ^ ((r & 0x8000u) ? 0x18005u : 0u);
    if ((b >> i) & 1u) r ^= a;
  }
  return r & 0xFFFFu;
}

__global__ __launch_bounds__(256) void flac_pack_k(const int16_t* __restrict__ pcm, const FlacRange* __restrict__ rng,
                                                   const FlacFrame* __restrict__ rec, const long long* __restrict__ off,
                                                   uint8_t* __restrict__ out, const long long* __restrict__ base) {
  __shared__ int s_x[FLAC_BLOCK + 4];
  __shared__ uint32_t s_w[FLAC_WORDS];
  __shared__ uint32_t s_scan[2][256];
  __shared__ uint32_t s_crc;
  const FlacRange R = rng[blockIdx.y];
  const long long slots = R.rate <= 0 ? 0 : (R.n + FLAC_BLOCK - 1) / FLAC_BLOCK;
  const long long f = blockIdx.x;
  if (f >= slots) return;
  const FlacFrame* fr = rec + R.frame0 + f;
  const int len = fr->len;
  if (len <= 0) return;
  const int t = threadIdx.x;
  const int n = fr->n, kind = fr->kind, o = fr->order, p = fr->part, hdr = fr->hdr;
  flac_load_block(pcm + R.start + f * FLAC_BLOCK, n, s_x);
  for (int i = t; i < FLAC_WORDS; i += 256) s_w[i] = 0;
  if (t == 0) s_crc = 0;
  __syncthreads();

  const uint32_t sub = 8u * (uint32_t)hdr;             // the subframe's first bit
  if (t == 0) {
    uint8_t h[16];
    int m = 0;
    const int rc = flac_rate_code(R.rate);
    h[m++] = 0xFF;
    h[m++] = base ? 0xF9 : 0xF8;                       // a stream's frames: variable block size, numbered by their first sample
    h[m++] = (uint8_t)(((n == FLAC_BLOCK ? 0xC : 0x7) << 4) | rc);
    h[m++] = 0x08;                                     // mono, 16 bits per sample
    const flac_u64 fn = flac_frame_number(base, blockIdx.y, f);
    const int nb = flac_number_bytes(fn);
    if (nb == 1) h[m++] = (uint8_t)fn;
    else {
      h[m++] = (uint8_t)(((0xFF << (8 - nb)) & 0xFF) | (uint32_t)(fn >> (6 * (nb - 1))));
      for (int i = nb - 2; i >= 0; --i) h[m++] = (uint8_t)(0x80 | ((uint32_t)(fn >> (6 * i)) & 0x3F));
    }
    if (n != FLAC_BLOCK) { h[m++] = (uint8_t)((n - 1) >> 8); h[m++] = (uint8_t)((n - 1) & 0xFF); }
    if (rc == 13) { h[m++] = (uint8_t)(R.rate >> 8); h[m++] = (uint8_t)(R.rate & 0xFF); }
    uint32_t c = 0;
    for (int i = 0; i < m; ++i) {
      c ^= h[i];
      for (int b = 0; b < 8; ++b) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    }
    h[m++] = (uint8_t)c;
    for (int i = 0; i < m; ++i) flac_put(s_w, 8u * i, h[i], 8);
    flac_put(s_w, sub, kind == 0 ? 0u : kind == 1 ? 2u : (uint32_t)((8 | o) << 1), 8);
    if (kind == 0) flac_put(s_w, sub + 8, (uint32_t)s_x[4] & 0xFFFFu, 16);
    if (kind == 2) {
      for (int i = 0; i < o; ++i) flac_put(s_w, sub + 8 + 16 * i, (uint32_t)s_x[4 + i] & 0xFFFFu, 16);
      flac_put(s_w, sub + 8 + 16 * o, (uint32_t)p, 6); // coding method 00, then the partition order
    }
  }
  const int i0 = t * 16, i1 = min(i0 + 16, n);
  if (kind == 1) {
    for (int i = i0; i < i1; ++i) flac_put(s_w, sub + 8 + 16u * i, (uint32_t)s_x[4 + i] & 0xFFFFu, 16);
  } else if (kind == 2) {
    const int S = n >> p;
    const int c1 = o == 0 ? 0 : o, c2 = o < 2 ? 0 : (o == 2 ? 1 : (o == 3 ? 3 : 6)), c3 = o < 3 ? 0 : (o == 3 ? 1 : 4), c4 = o == 4 ? 1 : 0;
    uint32_t total = 0;
    for (int i = max(i0, o); i < i1; ++i) {
      const uint32_t u = flac_zigzag(s_x[4 + i] - c1 * s_x[3 + i] + c2 * s_x[2 + i] - c3 * s_x[1 + i] + c4 * s_x[i]);
      const int k = fr->k[i / S];
      total += (u >> k) + 1 + k + ((i % S == 0 || i == o) ? 4 : 0);
    }
    int cur = 0;
    s_scan[0][t] = total;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      s_scan[cur ^ 1][t] = s_scan[cur][t] + (t >= d ? s_scan[cur][t - d] : 0);
      cur ^= 1;
      __syncthreads();
    }
    uint32_t pos = sub + 8 + 16 * o + 6 + s_scan[cur][t] - total;
    for (int i = max(i0, o); i < i1; ++i) {
      const uint32_t u = flac_zigzag(s_x[4 + i] - c1 * s_x[3 + i] + c2 * s_x[2 + i] - c3 * s_x[1 + i] + c4 * s_x[i]);
      const int k = fr->k[i / S];
      if (i % S == 0 || i == o) { flac_put(s_w, pos, (uint32_t)k, 4); pos += 4; }   // a partition's first residual: the parameter in front
      pos += u >> k;                                   // the unary run: the words are zero already
      flac_put(s_w, pos, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
      pos += k + 1;
    }
  }
  __syncthreads();

  {                                                    // CRC-16 over bytes [0, len - 2)
    const int L = len - 2, per = (L + 255) / 256;
    const int b0 = min(t * per, L), b1 = min(b0 + per, L);
    uint32_t c = 0;
    for (int b = b0; b < b1; ++b) {
      c ^= flac_byte(s_w, b) << 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
    }
    if (c) {
      uint32_t adv = 1, base = 0x0100u;                // x^8: one byte behind the piece
      for (int e = L - b1; e; e >>= 1) {
        if (e & 1) adv = flac_mulmod16(adv, base);
        base = flac_mulmod16(base, base);
      }
      atomicXor(&s_crc, flac_mulmod16(c, adv));
    }
    __syncthreads();
    if (t == 0) flac_put(s_w, 8u * L, s_crc, 16);
    __syncthreads();
  }

  uint8_t* dst = out + off[R.frame0 + f];
  const int a = (int)((uintptr_t)dst & 15);           // 16-byte units of the destination; unit m holds frame bytes [16 m - a, 16 m - a + 16)
  const int sh = 8 * ((16 - a) & 3);
  for (int m = t; 16 * m - a < len; m += 256) {
    const int q = 16 * m - a;
    if (q >= 0 && q + 16 <= len) {
      flac_u32x4 v;
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int wi = (q + 4 * j) >> 2;
        const uint32_t be = sh ? (s_w[wi] << sh) | (s_w[wi + 1] >> (32 - sh)) : s_w[wi];
        w[j] = __builtin_bswap32(be);
      }
      v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
      *reinterpret_cast<flac_u32x4*>(dst + q) = v;
    } else {
      for (int b = max(q, 0); b < min(q + 16, len); ++b) dst[b] = (uint8_t)flac_byte(s_w, b);
    }
  }
}

hipError_t launch_flac_encode(const int16_t* pcm, const long long* counts, const FlacRange* rng, int n_rng, long long frames_max,
                              long long n_frames, uint8_t* out, long long* meta, FlacFrame* rec, hipStream_t st) {
  if (n_rng <= 0 || frames_max <= 0 || n_frames <= 0) return hipSuccess;
  const dim3 grid((unsigned)frames_max, (unsigned)n_rng);
  hipLaunchKernelGGL(flac_analyse_k, grid, dim3(256), 0, st, pcm, counts, rng, rec, meta + n_frames + 1, (const long long*)nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flac_scan_k, dim3(1), dim3(1024), 0, st, (const FlacFrame*)rec, n_frames, meta);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flac_pack_k, grid, dim3(256), 0, st, pcm, rng, (const FlacFrame*)rec, (const long long*)meta, out,
                     (const long long*)nullptr);
  return hipGetLastError();
}

// ---- streams (ctts_flac_stream_step) -----------------------------------------------------------------------------------------------
// One workgroup per push: [the stream's carried samples | the push's samples, a final push's compacted by its keep mask] go to the
// push's 16-byte-aligned staging range, so that flac_load_block's aligned path serves the frames cut from it.  The cutting rule of
// chattts_amd/flac.py (stream_plan): blocks of 4096 from the front, a rest of 16 or more is one more block, a rest of 1 .. 15 waits in
// the stream's slot (state [slots][16] int16) unless the push is final.  The slot is read into LDS before the barrier and written
// behind it, by this workgroup alone (the host refuses a slot named twice).  A keep mask is MSB first and starts at byte start / 8.
// Thread 0 writes what the three encoder kernels read: the push's FlacRange over its staging range (its length the count written
// here), and the number of its first staged sample.
__global__ __launch_bounds__(1024) void flac_stage_k(const int16_t* __restrict__ pcm, const uint8_t* __restrict__ mask,
                                                     const long long* __restrict__ counts, const FlacPush* __restrict__ push,
                                                     int16_t* __restrict__ state, int16_t* __restrict__ stage, FlacRange* __restrict__ rng,
                                                     long long* __restrict__ base, long long* __restrict__ staged) {
  __shared__ int16_t s_c[FLAC_MIN_BLOCK];
  __shared__ int s_v[2][1024];
  __shared__ long long s_run;
  const FlacPush P = push[blockIdx.x];
  const int t = threadIdx.x;
  const int c = P.carry;
  const bool last = P.flags & 1, masked = P.flags & 2;
  int16_t* slot = state + (long long)P.slot * FLAC_MIN_BLOCK;
  if (t < FLAC_MIN_BLOCK) s_c[t] = t < c ? slot[t] : (int16_t)0;
  if (t == 0) s_run = 0;
  long long L = P.n;
  if (P.count_idx >= 0) {
    const long long k = counts[P.count_idx];
    L = k < 0 ? 0 : (k < L ? k : L);
  }
  __syncthreads();
  // a push that is not final has neither a count nor a mask: what it holds and emits is known before a sample is read
  const long long avail = c + L, r = avail & (FLAC_BLOCK - 1);
  const long long emit = last ? (1ll << 62) : avail < FLAC_MIN_BLOCK ? 0 : r < FLAC_MIN_BLOCK ? avail - r : avail;
  int16_t* dst = stage + P.stage;
  const int16_t* src = pcm + P.start;
  if (t < c) {
    dst[t] = s_c[t];
    if (t >= emit) slot[t - emit] = s_c[t];
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
    FlacRange R;
    R.start = P.stage;
    R.n = c + P.n;
    R.rate = P.rate;
    R.count_idx = (int32_t)blockIdx.x;
    R.frame0 = P.frame0;
    rng[blockIdx.x] = R;
    base[blockIdx.x] = P.sample;
    staged[blockIdx.x] = last ? held : emit;
  }
}

hipError_t launch_flac_stream(const int16_t* pcm, const uint8_t* mask, const long long* counts, const FlacPush* push, int n_push,
                              int16_t* state, long long frames_max, long long n_frames, uint8_t* out, long long* meta, long long* staged,
                              long long* base, FlacRange* rng, FlacFrame* rec, int16_t* stage, hipStream_t st) {
  if (n_push <= 0 || frames_max <= 0 || n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(flac_stage_k, dim3((unsigned)n_push), dim3(1024), 0, st, pcm, mask, counts, push, state, stage, rng, base, staged);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)frames_max, (unsigned)n_push);
  hipLaunchKernelGGL(flac_analyse_k, grid, dim3(256), 0, st, (const int16_t*)stage, (const long long*)staged, (const FlacRange*)rng, rec,
                     meta + n_frames + 1, (const long long*)base);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flac_scan_k, dim3(1), dim3(1024), 0, st, (const FlacFrame*)rec, n_frames, meta);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flac_pack_k, grid, dim3(256), 0, st, (const int16_t*)stage, (const FlacRange*)rng, (const FlacFrame*)rec,
                     (const long long*)meta, out, (const long long*)base);
  return hipGetLastError();
}
