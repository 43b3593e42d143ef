// G.711 companding on the device (ctts_g711_encode_ranges): 16-bit PCM -> one byte per sample, mu-law or A-law, strictly behind the PCM16
// conversion (codec.hip) -- the telephony form of every output path.  The map G is the ITU-T G.191 one (sign-symmetric: a negative sample
// is companded from its ONES' complement), chattts_amd/g711.py is its NumPy twin:
//   mu:  a = min((mag >> 2) + 33, 0x1FFF),  seg = 1 + bits(a >> 6),  code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)),  | 0x80 when lin >= 0
//   A:   ix = mag >> 4;  ix > 15: e = bits(ix) - 4, ix = ((ix >> (e - 1)) & 0xF) | (e << 4);  | 0x80 when lin >= 0;  ^ 0x55
// with mag = lin < 0 ? ~lin : lin and bits(v) = 32 - clz(v).  No branch depends on a sample.
// Table-driven like the window kernels: range r (G711Range) says that elements [start, start + n) of the int16 input become BYTES
// [start, start + n) of the output under `law` -- element offsets carry over with item size 1, so every host-side offset table of the
// PCM16 layouts is reused.  A workgroup takes a tile of G711_TILE samples of one range (blockIdx.y); a thread converts 16 consecutive
// samples: two 16-byte loads, one 16-byte store (starts are multiples of 8 elements: the loads are 16-byte aligned, the store 8-byte
// aligned).  Only a range's last partial group of 16 goes sample by sample.  Bytes outside every range and all bytes of a skipped range
// (law < 0) are not written.  Positions are 64-bit.
#include "common.hpp"
#include "kernels.hpp"

typedef int32_t g711_i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t g711_u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));

template <int LAW>
__device__ __forceinline__ uint32_t g711_code(int lin) {
  const int mag = lin ^ (lin >> 31);                       // lin < 0 ? ~lin : lin
  const uint32_t sign = ((uint32_t)~lin >> 24) & 0x80u;    // 0x80 when lin >= 0
  if (LAW == 0) {
    const int a = min((mag >> 2) + 33, 0x1FFF);
    const int seg = 33 - __clz(a >> 6);                    // 1 + significant bits of a >> 6 (__clz(0) = 32)
    return (uint32_t)(((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF))) | sign;
  }
  const int ix = mag >> 4;
  const int e = max(28 - __clz(ix), 0);                    // significant bits - 4: 0 for ix <= 15
  const int sh = max(e - 1, 0);
  return ((uint32_t)(((ix >> sh) & 0xF) | (e << 4)) | sign) ^ 0x55u;
}

template <int LAW>
__device__ __forceinline__ uint32_t g711_pack4(int w0, int w1) {   // two words of two int16 each -> four codes, sample order = byte order
  return g711_code<LAW>((int)(int16_t)(w0 & 0xFFFF)) | (g711_code<LAW>(w0 >> 16) << 8) | (g711_code<LAW>((int)(int16_t)(w1 & 0xFFFF)) << 16) |
         (g711_code<LAW>(w1 >> 16) << 24);
}

template <int LAW>
__device__ __forceinline__ void g711_group(const int16_t* __restrict__ src, uint8_t* __restrict__ dst, long long left) {
  if (left >= 16) {
    const g711_i32x4 a = *reinterpret_cast<const g711_i32x4*>(src);
    const g711_i32x4 b = *reinterpret_cast<const g711_i32x4*>(src + 8);
    g711_u32x4_a8 o;
    o.x = g711_pack4<LAW>(a.x, a.y);
    o.y = g711_pack4<LAW>(a.z, a.w);
    o.z = g711_pack4<LAW>(b.x, b.y);
    o.w = g711_pack4<LAW>(b.z, b.w);
    *reinterpret_cast<g711_u32x4_a8*>(dst) = o;
  } else {
#pragma clang loop vectorize(disable) unroll(disable)
    for (int j = 0; j < (int)left; ++j) dst[j] = (uint8_t)g711_code<LAW>((int)src[j]);   // the range's last partial group
  }
}

__global__ __launch_bounds__(256) void g711_ranges_k(const int16_t* __restrict__ pcm, uint8_t* __restrict__ out, const G711Range* __restrict__ rng) {
  const G711Range R = rng[blockIdx.y];
  if (R.law < 0) return;
  const long long i = (long long)blockIdx.x * G711_TILE + (long long)threadIdx.x * 16;   // the thread's first sample, relative to the range
  if (i >= R.n) return;
  const long long p = R.start + i;
  if (R.law == 0) g711_group<0>(pcm + p, out + p, R.n - i);
  else g711_group<1>(pcm + p, out + p, R.n - i);
}

hipError_t launch_g711_ranges(const int16_t* pcm, uint8_t* out, const G711Range* rng, int n_rng, long long n_max, hipStream_t st) {
  if (n_rng <= 0 || n_max <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n_max + G711_TILE - 1) / G711_TILE), (unsigned)n_rng);
  hipLaunchKernelGGL(g711_ranges_k, grid, dim3(256), 0, st, pcm, out, rng);
  return hipGetLastError();
}
