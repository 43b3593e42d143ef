// The dynamic range compressor on the device (ctts_compress_ragged): packed float32 segments, every segment compressed as if alone
// (chattts_amd/compressor.py holds the definition, the condition on the float64 sums and the NumPy twin).  Per segment at rate fs,
// B = fs / 1000 samples is a block of 1 ms:  p = the block's peak;  c = table[(bits(p) >> 18) - Q0], the static curve as data;
// m = the minimum of c over H blocks back and A blocks ahead;  s = the mean of m over A + 1 blocks (float64 sum, float64 division,
// one rounding);  a[b] = min(s[b - 1], s[b]);  g = a[b] + (a[b + 1] - a[b]) (t / B) in float64, every operation rounded once;  y = g x.
// The records are cleared by a memset node in front of two launches:
//  * compress_peak_k  -- a workgroup owns CP_PEAK_TILE blocks of one segment and stages the segment's table (4 KiB) in LDS.  A block
//    belongs to 4, 8 or 16 adjacent lanes (the float4s that cover B samples at any alignment: ceil((B + 3) / 4)): each lane loads 16
//    bytes at the pack's own alignment, masks what lies outside the block (single samples only at a segment's ragged edges), and a
//    cross-lane max over the group leaves the peak in its first lane, which looks c up and writes ONE float per block to the scratch.
//    A NaN compares false and does not count.  The record's block count goes by one integer atomic per workgroup, its peak by an
//    atomic max on the bits (p >= 0); min_gain = 1 is a plain store by the segment's first workgroup, ordered before the atomics of
//    the second launch by the kernel boundary.
//  * compress_apply_k -- a workgroup owns a sample tile of CP_TILE blocks of one segment.  It stages the c of the blocks its windows
//    reach (A + H + 1 in front, A + 1 behind, 1 outside the segment); where none is below 1 the tile's gain is 1 by the definition and
//    the workgroup copies (or, in place, leaves).  Otherwise the window minimum is taken in LDS by doubling, as in limiter.hip, s and
//    the anchors follow, t / B comes from a table of B quotients, and the gain is applied with 16-byte loads and stores.  min g goes
//    by an atomic min on the bits (g > 0) and the count of g < 1 by an integer atomic, one each per workgroup: neither depends on
//    order, so a record does not depend on what the segment is packed with.
// A segment whose table index is -1 is copied through with the record {1, 0, 0, 0}.  No fused multiply-add touches a gain: cp_gain
// switches contraction off.
//
// A STREAM (ctts_compress_stream_step; compressor.py: stream_plan): the segment arrives in pushes.  A slot carries the raw samples
// [emitted, pos), fewer than (A + 2) B, and the c of the blocks [h0, pos / B), at most 2 A + H + 2: the hold's memory is one float per
// millisecond, not samples.  Both are double-buffered by `phase`: a step reads one half and writes the other, so the workgroups that
// still read the old half in a launch never meet the write.  Two launches whatever the streams' number, rates, specs and push lengths:
//  * compress_stream_peak_k  -- compress_peak_k on the blocks the push completes (the partial last one too on the last push); the
//    first of them may begin in the slot's raw carry and go on in x.  The new c go to the step's scratch, one float per block.
//  * compress_stream_apply_k -- compress_apply_k on the blocks the step emits, by the same device functions (cp_tile_anchors, cp_gain):
//    a window's c come from the slot's history, then from the scratch; a sample from the raw carry (single loads: fewer than
//    (A + 2) B of a step), then from x (16-byte loads at x's own alignment, 16-byte stores where y's place allows).  The descriptor's
//    first workgroup also writes the slot's next raw carry and history into the other half; it runs when the step emits nothing, too.
// The slot's record lives across steps and is only ever touched by the order-free atomics of the two launches: the caller sets it to
// {1, 0, 0, 0} when the stream is opened, in stream order in front of its first step.
#include "common.hpp"
#include "kernels.hpp"

#define CP_NC (CP_TILE + 2 + 2 * CP_AMAX + CP_HMAX)      // the c values one sample tile can reach
#define CP_PER ((CP_NC + 255) / 256)
static_assert(CP_PER == 3 && CP_TABLE == 4 * 256, "three staged values per thread; the table is one float4 per thread");
static_assert((unsigned long long)(CP_TILE * CP_BMAX) * ((1u << 20) / CP_BMIN + 1) < (1ull << 32), "r * M stays in 32 bits");

struct CpStats {        // compressor.STATS
  float min_gain;
  int32_t n_blocks, n_touched;
  float peak;
};
static_assert(sizeof(CpStats) == 16, "compressor.STATS is 16 bytes");

__device__ __forceinline__ int cp_block_sum(int v, int* red, int tid) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
// |v| into the running peak; false for a NaN, which does not count
__device__ __forceinline__ float cp_peak(float p, float v) {
  const float a = fabsf(v);
  return a > p ? a : p;
}
// lane l of a block's lanes: the peak of its float4 of the samples [bs, be) of x -- 16 bytes at x's own alignment, masked to the block,
// where the float4 lies inside [lo, hi), what may be loaded; single samples at the ragged edges
__device__ __forceinline__ float cp_span_peak(const float* __restrict__ x, long long bs, long long be, long long lo, long long hi, int l) {
  const long long p = (bs & ~3ll) + 4 * l;
  float v = 0.0f;
  if (p < be) {
    if (p >= lo && p + 4 <= hi) {
      const float4 q = *reinterpret_cast<const float4*>(x + p);
      if (p >= bs) v = cp_peak(v, q.x);
      if (p + 1 >= bs && p + 1 < be) v = cp_peak(v, q.y);
      if (p + 2 >= bs && p + 2 < be) v = cp_peak(v, q.z);
      if (p + 3 >= bs && p + 3 < be) v = cp_peak(v, q.w);
    } else {
      for (long long k = max(p, bs); k < min(p + 4, be); ++k) v = cp_peak(v, x[k]);
    }
  }
  return v;
}
// step 3: c of a block peak (p >= 0, not NaN), the table staged in LDS
__device__ __forceinline__ float cp_curve(const float* tab, float p) {
  const int q = (int)(__float_as_uint(p) >> 18) - CP_Q0;
  return q < 0 ? 1.0f : tab[min(q, CP_TABLE - 1)];
}

__global__ __launch_bounds__(256) void compress_peak_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                       const int32_t* __restrict__ rate, const int32_t* __restrict__ par,
                                                       const float* __restrict__ tabs, float* __restrict__ cb, CpStats* stats) {
  __shared__ float tab[CP_TABLE];
  __shared__ int red[4];
  __shared__ float redf[4];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int ti = par[4 * s + 2];
  const long long lo = off[s], hi = off[s + 1];
  const int B = rate[s] / 1000;
  const long long nb = (hi - lo + B - 1) / B, b0 = (long long)blockIdx.x * CP_PEAK_TILE;
  if (b0 >= nb) return;
  if (blockIdx.x == 0 && tid == 0) stats[s].min_gain = 1.0f;
  if (ti < 0) return;                                               // copied through: the record stays {1, 0, 0, 0}
  reinterpret_cast<float4*>(tab)[tid] = reinterpret_cast<const float4*>(tabs + (size_t)ti * CP_TABLE)[tid];
  __syncthreads();
  const int G = B <= 13 ? 4 : B <= 29 ? 8 : 16;                     // lanes per block: ceil((B + 3) / 4) float4s cover it
  const int per = 256 / G, grp = tid / G, l = tid % G;
  const int nbt = (int)min((long long)CP_PEAK_TILE, nb - b0);
  float* cs = cb + lo / CP_BMIN + s;
  float pmax = 0.0f;
  int cnt = 0;
  for (int base = 0; base < nbt; base += per) {                     // workgroup-uniform: every lane takes part in the shuffles
    const int bi = base + grp;
    const long long bs = lo + (b0 + bi) * B, be = min(bs + B, hi);
    float v = bi < nbt ? cp_span_peak(x, bs, be, lo, hi, l) : 0.0f;
    for (int m = 1; m < G; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));   // no NaN left: v >= 0
    if (bi < nbt && l == 0) {
      const float c = cp_curve(tab, v);
      cs[b0 + bi] = c;
      cnt += c < 1.0f;
      pmax = fmaxf(pmax, v);
    }
  }
  for (int m = 32; m >= 1; m >>= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, m, 64));
  if ((tid & 63) == 0) redf[tid >> 6] = pmax;
  cnt = cp_block_sum(cnt, red, tid);                                // its barrier publishes redf as well
  if (tid == 0) {
    if (cnt) atomicAdd(&stats[s].n_blocks, cnt);
    pmax = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    if (pmax > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(&stats[s].peak), __float_as_uint(pmax));
  }
}

// samples [s0, s1) of the pack, y = x: 16 bytes at the pack's own alignment, single samples at the ragged edges
__device__ __forceinline__ void cp_copy(const float* x, float* y, long long s0, long long s1, int tid) {
  if (x == y) return;
  for (long long p = (s0 & ~3ll) + 4 * tid; p < s1; p += 1024) {
    if (p >= s0 && p + 4 <= s1) {
      *reinterpret_cast<float4*>(y + p) = *reinterpret_cast<const float4*>(x + p);
    } else {
      for (long long k = max(p, s0); k < min(p + 4, s1); ++k) y[k] = x[k];
    }
  }
}
// step 6 of the definition: the difference (exact), the product and the sum in float64, each rounded once, then one rounding to float32.
// The __d*_rn intrinsics are plain operators in the HIP headers and carry the translation unit's permission to contract, so the operators
// are written out with contraction switched off: v_mul_f64 and v_add_f64, never a v_fma_f64 (NumPy cannot fuse)
__device__ __forceinline__ float cp_gain(const double* an, const double* frac, unsigned r, unsigned M, int B) {
#pragma clang fp contract(off)
  const unsigned bl = (r * M) >> 20;                                // r / B for r < CP_TILE * CP_BMAX, M = ceil(2^20 / B)
  const double a0 = an[bl];
  const double d = an[bl + 1] - a0;
  const double q = d * frac[r - bl * B];
  return __double2float_rn(a0 + q);
}

// Steps 4 .. 6 up to the anchors, for the sample tile of the blocks [b0, b0 + nbt) of a signal of nb blocks: c_of(k) is c of block k
// (1 outside 0 <= k < nb, the functor's to say).  Stages the c the tile's windows reach; where none is below 1 the tile's gain is 1 by
// the definition and the function returns false at once (the caller copies).  Otherwise: the window minimum in LDS by doubling, s, the
// quotients t / B and the anchors an[0 .. nbt] of the blocks [b0, b0 + nbt] (s[-1] := s[0], a[nb] := s[nb - 1]) -> true.  Every thread
// of the workgroup calls it: it holds barriers.  a [CP_NC], sv [CP_TILE + 2], an [CP_TILE + 1], frac [CP_BMAX]
template <class COf>
__device__ __forceinline__ bool cp_tile_anchors(float* a, float* sv, double* an, double* frac, int tid, long long b0, int nbt, long long nb,
                                                int A, int H, int B, COf c_of) {
  const int nc = nbt + 2 + 2 * A + H, nm = nbt + 2 + A, L = A + H + 1;
  // c over the blocks [b0 - 1 - A - H, b0 + nbt + A]: a[e] is block b0 - 1 - A - H + e, 1 outside the segment
  float v[CP_PER];
  int any = 0;
#pragma unroll
  for (int i = 0; i < CP_PER; ++i) {
    const int e = tid + 256 * i;
    v[i] = e < nc ? c_of(b0 - 1 - A - H + e) : 1.0f;
    if (e < nc) a[e] = v[i];
    any |= v[i] < 1.0f;
  }
  if (!__syncthreads_or(any)) return false;                         // no block below 1 in reach: m, s, a and g are 1 on the whole tile
  int p = 1;
  for (; 2 * p <= L; p *= 2) {                                      // a[e] = min c over [e, e + p)  ->  over [e, e + 2 p)
#pragma unroll
    for (int i = 0; i < CP_PER; ++i) {
      const int e = tid + 256 * i;
      if (e < nc) v[i] = e + p < nc ? fminf(a[e], a[e + p]) : a[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CP_PER; ++i) {
      const int e = tid + 256 * i;
      if (e < nc) a[e] = v[i];
    }
    __syncthreads();
  }
  // m over the blocks [b0 - 1 - A, b0 + nbt]: a[e] = min c over [e, e + L);  e + L - p + p <= nm - 1 + L = nc - 1 + 1
#pragma unroll
  for (int i = 0; i < CP_PER; ++i) {
    const int e = tid + 256 * i;
    if (e < nm) v[i] = fminf(a[e], a[e + L - p]);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CP_PER; ++i) {
    const int e = tid + 256 * i;
    if (e < nm) a[e] = v[i];
  }
  __syncthreads();
  if (tid < nbt + 2) {                                              // s over the blocks [b0 - 1, b0 + nbt]: the sum is exact in any order
    double S = 0.0;
    for (int d = 0; d <= A; ++d) S = __dadd_rn(S, (double)a[tid + d]);
    sv[tid] = __double2float_rn(__ddiv_rn(S, (double)(A + 1)));
  }
  if (tid < B) frac[tid] = __ddiv_rn((double)tid, (double)B);
  __syncthreads();
  if (tid <= nbt) {                                                 // anchors of the blocks [b0, b0 + nbt]; s[-1] := s[0], a[nb] := s[nb - 1]
    const long long b = b0 + tid;
    const int i0 = (int)(max(b - 1, 0ll) - b0) + 1, i1 = (int)(min(b, nb - 1) - b0) + 1;
    an[tid] = (double)fminf(sv[i0], sv[i1]);
  }
  __syncthreads();
  return true;
}
// the tile's smallest gain and its count of g < 1 into the record: one atomic each per workgroup, neither depends on order
__device__ __forceinline__ void cp_tile_record(float mn, int touched, int* red, float* redf, int tid, CpStats* st) {
  for (int m = 32; m >= 1; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m, 64));
  if ((tid & 63) == 0) redf[tid >> 6] = mn;
  touched = cp_block_sum(touched, red, tid);                        // its barrier publishes redf as well
  if (tid == 0 && touched) {
    atomicAdd(&st->n_touched, touched);
    atomicMin(reinterpret_cast<unsigned int*>(&st->min_gain), __float_as_uint(fminf(fminf(redf[0], redf[1]), fminf(redf[2], redf[3]))));
  }
}

__global__ __launch_bounds__(256) void compress_apply_k(const float* x, float* y, const long long* __restrict__ off,
                                                        const int32_t* __restrict__ rate, const int32_t* __restrict__ par,
                                                        const float* __restrict__ cb, CpStats* stats) {
  __shared__ float a[CP_NC];
  __shared__ float sv[CP_TILE + 2];
  __shared__ double an[CP_TILE + 1];
  __shared__ double frac[CP_BMAX];
  __shared__ int red[4];
  __shared__ float redf[4];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long long lo = off[s], hi = off[s + 1];
  const int B = rate[s] / 1000;
  const long long nb = (hi - lo + B - 1) / B, b0 = (long long)blockIdx.x * CP_TILE;
  if (b0 >= nb) return;
  const int nbt = (int)min((long long)CP_TILE, nb - b0);
  const long long s0 = lo + b0 * B, s1 = min(s0 + (long long)nbt * B, hi);
  if (par[4 * s + 2] < 0) {                                         // copied through
    cp_copy(x, y, s0, s1, tid);
    return;
  }
  const float* cs = cb + lo / CP_BMIN + s;
  if (!cp_tile_anchors(a, sv, an, frac, tid, b0, nbt, nb, par[4 * s], par[4 * s + 1], B,
                       [&](long long k) { return k >= 0 && k < nb ? cs[k] : 1.0f; })) {
    cp_copy(x, y, s0, s1, tid);
    return;
  }
  const unsigned M = ((1u << 20) + B - 1) / B;
  float mn = 1.0f;
  int touched = 0;
  for (long long q = (s0 & ~3ll) + 4 * tid; q < s1; q += 1024) {
    if (q >= s0 && q + 4 <= s1) {
      const float4 in = *reinterpret_cast<const float4*>(x + q);
      const unsigned r = (unsigned)(q - s0);
      const float g0 = cp_gain(an, frac, r, M, B), g1 = cp_gain(an, frac, r + 1, M, B), g2 = cp_gain(an, frac, r + 2, M, B),
                  g3 = cp_gain(an, frac, r + 3, M, B);
      *reinterpret_cast<float4*>(y + q) = make_float4(__fmul_rn(g0, in.x), __fmul_rn(g1, in.y), __fmul_rn(g2, in.z), __fmul_rn(g3, in.w));
      mn = fminf(fminf(mn, fminf(g0, g1)), fminf(g2, g3));
      touched += (g0 < 1.0f) + (g1 < 1.0f) + (g2 < 1.0f) + (g3 < 1.0f);
    } else {
      for (long long k = max(q, s0); k < min(q + 4, s1); ++k) {
        const float g = cp_gain(an, frac, (unsigned)(k - s0), M, B);
        y[k] = __fmul_rn(g, x[k]);
        mn = fminf(mn, g);
        touched += g < 1.0f;
      }
    }
  }
  cp_tile_record(mn, touched, red, redf, tid, &stats[s]);
}

// ---- streams --------------------------------------------------------------------------------------------------------------------------
static_assert(CP_SCARRY >= (CP_AMAX + 2) * CP_BMAX && CP_SHIST >= 2 * CP_AMAX + CP_HMAX + 2 && CP_SCARRY % 4 == 0 && CP_SHIST % 4 == 0,
              "a slot keeps fewer than (A + 2) B raw samples and at most 2 A + H + 2 block gains");

// what the kernels derive from a descriptor (the C entry has checked every count against compressor.py's stream_plan)
struct CpStreamView {
  int B;
  bool fin;
  long long pos, end, e_lo, e_hi, nbc0, nbc1, h0;                   // samples in before / behind the push; emitted before / behind; blocks with a c before / behind; the first block of the history
  const float *xin, *raw, *hist, *cnew;                             // x at sample pos; the slot's raw carry at sample e_lo; its c at block h0; the step's c at block nbc0
  __device__ __forceinline__ CpStreamView(const CpStream& D, const float* x, const float* carry, const float* hold, const float* cb) {
    B = D.rate / 1000;
    fin = D.total >= 0;
    pos = D.pos; end = D.pos + D.n_in; e_lo = D.e_lo; e_hi = D.e_lo + D.n_out;
    nbc0 = pos / B; nbc1 = fin ? (end + B - 1) / B : end / B; h0 = nbc0 - D.h_in;
    xin = x + D.in_off;
    raw = carry + ((long long)D.slot * 2 + D.phase) * CP_SCARRY;
    hist = hold ? hold + ((long long)D.slot * 2 + D.phase) * CP_SHIST : nullptr;           // the peak launch reads no history
    cnew = cb + D.cb_off;
  }
  // sample g of the stream, e_lo <= g < end: the raw carry, then the push
  __device__ __forceinline__ float sample(long long g) const { return g >= pos ? xin[g - pos] : raw[g - e_lo]; }
  // c of block k: the history, then the step's new blocks; 1 outside the signal (beyond nbc1 on the last push only: before it no window reaches there)
  __device__ __forceinline__ float c_of(long long k) const {
    if (k < 0 || k >= nbc1) return 1.0f;
    return k >= nbc0 ? cnew[k - nbc0] : hist[k - h0];
  }
};

__global__ __launch_bounds__(256) void compress_stream_peak_k(const float* __restrict__ x, const CpStream* __restrict__ tab,
                                                              const float* __restrict__ tabs, const float* __restrict__ carry,
                                                              float* __restrict__ cb, CpStats* stats) {
  __shared__ float tb[CP_TABLE];
  __shared__ int red[4];
  __shared__ float redf[4];
  const CpStream& D = tab[blockIdx.y];
  const int tid = threadIdx.x;
  const CpStreamView V(D, x, carry, nullptr, cb);
  const int B = V.B;
  const long long nbn = V.nbc1 - V.nbc0, t0 = (long long)blockIdx.x * CP_PEAK_TILE;   // the blocks the push completes; the tile's first among them
  if (t0 >= nbn) return;
  reinterpret_cast<float4*>(tb)[tid] = reinterpret_cast<const float4*>(tabs + (size_t)D.tab * CP_TABLE)[tid];
  __syncthreads();
  const int G = B <= 13 ? 4 : B <= 29 ? 8 : 16;                     // lanes per block, as in compress_peak_k
  const int per = 256 / G, grp = tid / G, l = tid % G;
  const int nbt = (int)min((long long)CP_PEAK_TILE, nbn - t0);
  const long long xlo = D.in_off, xhi = D.in_off + D.n_in;          // the push in x: what may be loaded
  float pmax = 0.0f;
  int cnt = 0;
  for (int base = 0; base < nbt; base += per) {                     // workgroup-uniform: every lane takes part in the shuffles
    const int bi = base + grp;
    const long long bs = (V.nbc0 + t0 + bi) * B, be = min(bs + B, V.end);
    float v = 0.0f;
    if (bi < nbt) {
      const long long xs = max(bs, V.pos);                          // [bs, xs) lies in the raw carry: the block that was open, no other
      if (xs < be) v = cp_span_peak(x, xlo + (xs - V.pos), xlo + (be - V.pos), xlo, xhi, l);
      for (long long k = bs + l; k < min(xs, be); k += G) v = cp_peak(v, V.raw[k - V.e_lo]);
    }
    for (int m = 1; m < G; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    if (bi < nbt && l == 0) {
      const float c = cp_curve(tb, v);
      cb[D.cb_off + t0 + bi] = c;
      cnt += c < 1.0f;
      pmax = fmaxf(pmax, v);
    }
  }
  for (int m = 32; m >= 1; m >>= 1) pmax = fmaxf(pmax, __shfl_xor(pmax, m, 64));
  if ((tid & 63) == 0) redf[tid >> 6] = pmax;
  cnt = cp_block_sum(cnt, red, tid);                                // its barrier publishes redf as well
  if (tid == 0) {
    CpStats* st = stats + D.slot;
    if (cnt) atomicAdd(&st->n_blocks, cnt);
    pmax = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    if (pmax > 0.0f) atomicMax(reinterpret_cast<unsigned int*>(&st->peak), __float_as_uint(pmax));
  }
}

__global__ __launch_bounds__(256) void compress_stream_apply_k(const float* __restrict__ x, const CpStream* __restrict__ tab,
                                                               float* __restrict__ y, float* __restrict__ carry, float* __restrict__ hold,
                                                               const float* __restrict__ cb, CpStats* stats) {
  __shared__ float a[CP_NC];
  __shared__ float sv[CP_TILE + 2];
  __shared__ double an[CP_TILE + 1];
  __shared__ double frac[CP_BMAX];
  __shared__ int red[4];
  __shared__ float redf[4];
  const CpStream& D = tab[blockIdx.y];
  const int tid = threadIdx.x;
  const CpStreamView V(D, x, carry, hold, cb);
  const int B = V.B;
  const long long eb0 = V.e_lo / B, neb = (D.n_out + B - 1) / B;    // the blocks the step emits: [eb0, eb0 + neb), whole but for the signal's last
  const long long t0 = (long long)blockIdx.x * CP_TILE;
  const bool has = t0 < neb;
  if (!has && blockIdx.x != 0) return;                              // the whole workgroup: nothing waits at a barrier
  if (blockIdx.x == 0 && !V.fin) {                                  // more to come: the other half gets samples [e_hi, end) and the c of [h1, nbc1)
    float* raw1 = carry + ((long long)D.slot * 2 + (D.phase ^ 1)) * CP_SCARRY;
    float* hist1 = hold + ((long long)D.slot * 2 + (D.phase ^ 1)) * CP_SHIST;
    const long long h1 = V.nbc1 - D.h_out;                          // >= h0: a history never reaches back beyond the one before it
    for (int i = tid; i < D.c_out; i += 256) raw1[i] = V.sample(V.e_hi + i);
    for (int i = tid; i < D.h_out; i += 256) hist1[i] = V.c_of(h1 + i);
  }
  if (!has) return;                                                 // workgroup-uniform
  const long long b0 = eb0 + t0;
  const int nbt = (int)min((long long)CP_TILE, neb - t0);
  const long long s0 = b0 * B, s1 = min(s0 + (long long)nbt * B, V.e_hi);
  float* yw = y + D.out_off;                                        // sample g of the stream goes to yw[g - e_lo]
  // the tile's samples come from two sources: [s0, sx) from the slot's raw carry (fewer than (A + 2) B of a step, single samples), [sx, s1)
  // from the push -- 16-byte loads at x's own alignment as in compress_apply_k, and 16-byte stores where the chunk's place in y allows
  const long long sx = min(max(s0, V.pos), s1);
  const long long xo = D.in_off - V.pos;                            // sample g >= pos is x[g + xo]
  const bool st16 = (((uintptr_t)yw + 4 * (uintptr_t)(((sx + xo) & ~3ll) - xo - V.e_lo)) & 15) == 0;   // a 16-byte load's four samples go to a 16-byte place
  if (!cp_tile_anchors(a, sv, an, frac, tid, b0, nbt, V.nbc1, D.A, D.H, B, [&](long long k) { return V.c_of(k); })) {
    for (long long g = s0 + tid; g < sx; g += 256) yw[g - V.e_lo] = V.raw[g - V.e_lo];
    for (long long q = ((sx + xo) & ~3ll) + 4 * tid; q < s1 + xo; q += 1024) {
      if (q >= sx + xo && q + 4 <= s1 + xo) {
        const float4 in = *reinterpret_cast<const float4*>(x + q);
        float* o = yw + (q - xo - V.e_lo);
        if (st16) *reinterpret_cast<float4*>(o) = in;
        else { o[0] = in.x; o[1] = in.y; o[2] = in.z; o[3] = in.w; }
      } else {
        for (long long k = max(q, sx + xo); k < min(q + 4, s1 + xo); ++k) yw[k - xo - V.e_lo] = x[k];
      }
    }
    return;
  }
  const unsigned M = ((1u << 20) + B - 1) / B;
  float mn = 1.0f;
  int touched = 0;
  for (long long g = s0 + tid; g < sx; g += 256) {
    const float gn = cp_gain(an, frac, (unsigned)(g - s0), M, B);
    yw[g - V.e_lo] = __fmul_rn(gn, V.raw[g - V.e_lo]);
    mn = fminf(mn, gn);
    touched += gn < 1.0f;
  }
  for (long long q = ((sx + xo) & ~3ll) + 4 * tid; q < s1 + xo; q += 1024) {
    if (q >= sx + xo && q + 4 <= s1 + xo) {
      const float4 in = *reinterpret_cast<const float4*>(x + q);
      const unsigned r = (unsigned)(q - xo - s0);
      const float g0 = cp_gain(an, frac, r, M, B), g1 = cp_gain(an, frac, r + 1, M, B), g2 = cp_gain(an, frac, r + 2, M, B),
                  g3 = cp_gain(an, frac, r + 3, M, B);
      const float4 out = make_float4(__fmul_rn(g0, in.x), __fmul_rn(g1, in.y), __fmul_rn(g2, in.z), __fmul_rn(g3, in.w));
      float* o = yw + (q - xo - V.e_lo);
      if (st16) *reinterpret_cast<float4*>(o) = out;
      else { o[0] = out.x; o[1] = out.y; o[2] = out.z; o[3] = out.w; }
      mn = fminf(fminf(mn, fminf(g0, g1)), fminf(g2, g3));
      touched += (g0 < 1.0f) + (g1 < 1.0f) + (g2 < 1.0f) + (g3 < 1.0f);
    } else {
      for (long long k = max(q, sx + xo); k < min(q + 4, s1 + xo); ++k) {
        const float gn = cp_gain(an, frac, (unsigned)(k - xo - s0), M, B);
        yw[k - xo - V.e_lo] = __fmul_rn(gn, x[k]);
        mn = fminf(mn, gn);
        touched += gn < 1.0f;
      }
    }
  }
  cp_tile_record(mn, touched, red, redf, tid, stats + D.slot);
}

hipError_t launch_compress_stream(const float* x, const CpStream* tab, int n_streams, long long nb_new_max, long long nb_out_max,
                                  const float* tabs, float* y, float* carry, float* hold, void* stats, float* cb, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  if (nb_new_max > 0) {
    hipLaunchKernelGGL(compress_stream_peak_k, dim3((unsigned)((nb_new_max + CP_PEAK_TILE - 1) / CP_PEAK_TILE), (unsigned)n_streams), dim3(256),
                       0, st, x, tab, tabs, carry, cb, (CpStats*)stats);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // at least one workgroup per descriptor: a step that emits nothing still moves the carry and the history
  const long long tiles = (nb_out_max + CP_TILE - 1) / CP_TILE;
  hipLaunchKernelGGL(compress_stream_apply_k, dim3((unsigned)(tiles > 0 ? tiles : 1), (unsigned)n_streams), dim3(256), 0, st, x, tab, y, carry,
                     hold, cb, (CpStats*)stats);
  return hipGetLastError();
}

hipError_t launch_compress_ragged(const float* x, float* y, const long long* off, int n_seg, long long nb_max, const int32_t* rate,
                                  const int32_t* par, const float* tabs, void* stats, float* cb, hipStream_t st) {
  if (n_seg <= 0 || nb_max <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(CpStats) * (size_t)n_seg, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(compress_peak_k, dim3((unsigned)((nb_max + CP_PEAK_TILE - 1) / CP_PEAK_TILE), (unsigned)n_seg), dim3(256), 0, st, x, off,
                     rate, par, tabs, cb, (CpStats*)stats);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(compress_apply_k, dim3((unsigned)((nb_max + CP_TILE - 1) / CP_TILE), (unsigned)n_seg), dim3(256), 0, st, x, y, off, rate,
                     par, cb, (CpStats*)stats);
  return hipGetLastError();
}
