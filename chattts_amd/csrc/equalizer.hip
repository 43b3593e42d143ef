// The output equaliser on the device (ctts_equalize_ragged): packed float32 segments, every segment through its own cascade of up to
// four biquads as if alone (chattts_amd/equalizer.py holds the definition, the route and its NumPy twin).  The cascade is a linear system
// of D = 2 nsec states, s' = A s + B x (eq_step is one sample of it, transposed direct form II, float64 throughout), so a 10 s segment at
// 48 kHz, a 480,000-step chain, is computed exactly and in parallel.  A segment is cut into tiles of EQ_TILE = 64 EQ_CHUNK samples
// anchored at the segment's first sample -- never at the pack's, so a segment's result does not depend on what it is packed with -- and a
// wave owns a tile: it stages it in LDS by coalesced loads, and lane l owns the chunk [l c, (l + 1) c), c = EQ_CHUNK = 33 (odd: the lanes'
// reads at stride c fall on 32 different banks).  Three launches:
//  * equalize_state_k -- every tile but a segment's last (nothing reads that one's end state; a segment of one tile launches nothing
//    here).  Each lane runs its chunk from zero state; six shuffle steps scan the chunks' end states with A^(c 2^k) (host table); lane 63
//    then holds the tile's end state under a zero entry, z_T, and writes it to the tile's record (8 float64).
//  * equalize_scan_k  -- one wave per segment: the true entry states e_{T+1} = A^TILE e_T + z_T, in batches of 63 tiles, a tile per
//    lane behind lane 0, which holds the state behind the batch before: the same six shuffle steps with A^(TILE 2^k) scan the batch,
//    and record T comes back holding e_{T+1}.  A 10 s segment at 48 kHz is 227 records: four batches, not 227 steps in a row.
//  * equalize_apply_k -- every tile.  Lane 0 runs its chunk from the tile's true entry state (record T - 1; zero for the first tile), the
//    others from zero; the same scan now leaves every chunk's TRUE end state, one shuffle hands each lane its entry state, and the lane
//    runs its chunk again from it, rounds every output once to float32 into the staged tile, which the wave stores coalesced.  y may be x:
//    a wave writes only the tile it has staged, and equalize_state_k has read what it needs before this launch begins.
// Three passes over the samples -- one read of x per launch that touches them and one write -- and no per-sample table.  A segment whose
// row index is -1 is copied through bit for bit (left alone in place).  The cascade's length is a template parameter, chosen per
// segment by a workgroup-uniform switch: a one-section preset does a quarter of the four-section work.
#include "common.hpp"
#include "kernels.hpp"

static_assert(EQ_TILE == 64 * EQ_CHUNK && (EQ_CHUNK & 1) == 1 && EQ_D == 2 * EQ_NSEC, "a tile is 64 odd chunks; two states per section");
static_assert(EQ_ROW >= 32 + 12 * EQ_D * EQ_D && 4 + 5 * EQ_NSEC <= 32, "a row holds the header, the coefficients and twelve D x D matrices");
static_assert((size_t)EQ_WAVES * EQ_TILE * sizeof(float) <= 65536, "the staged tiles fit the LDS a launch gets without asking");

// one sample of a cascade of NS sections; k: b0 b1 b2 a1 a2 per section
template <int NS>
__device__ __forceinline__ double eq_step(const double (&k)[5 * NS], double x, double (&s)[2 * NS]) {
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const double y = fma(k[5 * i], x, s[2 * i]);
    s[2 * i] = fma(-k[5 * i + 3], y, fma(k[5 * i + 1], x, s[2 * i + 1]));
    s[2 * i + 1] = fma(-k[5 * i + 4], y, k[5 * i + 2] * x);
    x = y;
  }
  return x;
}
// inclusive scan over the wave's chunks: S_l = sum_{m <= l} A^(c (l - m)) z_m; P: the row's matrices A^(c 2^j), 8 x 8 row-major.  Every
// lane in front of the last one with samples ran a full chunk, so its S is the state behind its chunk; what the lanes from that one on
// hold is never read
template <int NS>
__device__ __forceinline__ void eq_scan(const double* __restrict__ P, int l, double (&s)[2 * NS]) {
  constexpr int D = 2 * NS;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int d = 1 << j;
    const double* Pd = P + j * EQ_D * EQ_D;
    double u[D];
#pragma unroll
    for (int q = 0; q < D; ++q) u[q] = __shfl_up(s[q], d, 64);
    if (l >= d) {
#pragma unroll
      for (int r = 0; r < D; ++r) {
        double a = s[r];
#pragma unroll
        for (int q = 0; q < D; ++q) a = fma(Pd[r * EQ_D + q], u[q], a);
        s[r] = a;
      }
    }
  }
}

// a full tile from zero state: its end state under a zero entry -> out[0 .. EQ_D), zeros beyond D
template <int NS>
__device__ __forceinline__ void eq_state(const double* __restrict__ R, const float* tw, int l, double* __restrict__ out) {
  constexpr int D = 2 * NS;
  double k[5 * NS], s[D];
#pragma unroll
  for (int i = 0; i < 5 * NS; ++i) k[i] = R[4 + i];
#pragma unroll
  for (int q = 0; q < D; ++q) s[q] = 0.0;
  const float* tc = tw + l * EQ_CHUNK;
  for (int i = 0; i < EQ_CHUNK; ++i) eq_step<NS>(k, (double)tc[i], s);
  eq_scan<NS>(R + 32, l, s);
  if (l == 63) {
#pragma unroll
    for (int q = 0; q < D; ++q) out[q] = s[q];
#pragma unroll
    for (int q = D; q < EQ_D; ++q) out[q] = 0.0;                    // the scan reads all eight
  }
}

// a tile of tl samples (0: the wave has none, it only takes part in the shuffles) from its entry state (null: zero): the outputs,
// rounded once to float32, replace the samples in tw
template <int NS>
__device__ __forceinline__ void eq_apply(const double* __restrict__ R, float* tw, int tl, int l, const double* __restrict__ entry) {
  constexpr int D = 2 * NS;
  double k[5 * NS], s[D], e[D];
#pragma unroll
  for (int i = 0; i < 5 * NS; ++i) k[i] = R[4 + i];
#pragma unroll
  for (int q = 0; q < D; ++q) e[q] = entry ? entry[q] : 0.0;
#pragma unroll
  for (int q = 0; q < D; ++q) s[q] = l == 0 ? e[q] : 0.0;
  float* tc = tw + l * EQ_CHUNK;
  const int len = max(0, min(EQ_CHUNK, tl - l * EQ_CHUNK));
  for (int i = 0; i < len; ++i) eq_step<NS>(k, (double)tc[i], s);
  eq_scan<NS>(R + 32, l, s);
#pragma unroll
  for (int q = 0; q < D; ++q) {
    const double up = __shfl_up(s[q], 1, 64);
    s[q] = l == 0 ? e[q] : up;
  }
  for (int i = 0; i < len; ++i) tc[i] = __double2float_rn(eq_step<NS>(k, (double)tc[i], s));
}

__global__ __launch_bounds__(64 * EQ_WAVES) void equalize_state_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                                  const int32_t* __restrict__ sel, const double* __restrict__ coef,
                                                                  double* __restrict__ rec) {
  __shared__ float tile[EQ_WAVES * EQ_TILE];
  const int s = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int ri = sel[s];
  if (ri < 0) return;                                               // copied through (the whole workgroup)
  const long long lo = off[s], n = off[s + 1] - lo;
  const long long nt = (n + EQ_TILE - 1) / EQ_TILE;
  const long long j = (long long)blockIdx.x * EQ_WAVES + w;         // this wave's tile of the segment
  if ((long long)blockIdx.x * EQ_WAVES + 1 >= nt) return;           // no wave of this workgroup has a tile in front of the last
  const bool has = j + 1 < nt;                                      // a full tile, and one whose end state is read
  float* tw = tile + w * EQ_TILE;
  if (has) {
    const float* xs = x + lo + j * EQ_TILE;
    for (int i = l; i < EQ_TILE; i += 64) tw[i] = xs[i];
  }
  __syncthreads();                                                  // the only barrier: a wave without a tile leaves behind it
  if (!has) return;
  const double* R = coef + (long long)ri * EQ_ROW;
  double* out = rec + (lo / EQ_TILE + s + j) * EQ_D;
  switch ((int)R[0]) {
    case 1: eq_state<1>(R, tw, l, out); break;
    case 2: eq_state<2>(R, tw, l, out); break;
    case 3: eq_state<3>(R, tw, l, out); break;
    default: eq_state<4>(R, tw, l, out); break;
  }
}

__global__ __launch_bounds__(64) void equalize_scan_k(const long long* __restrict__ off, const int32_t* __restrict__ sel,
                                                      const double* __restrict__ coef, double* __restrict__ rec) {
  __shared__ double PT[6 * EQ_D * EQ_D];                            // A^(TILE 2^k), k = 0 .. 5, staged: held in scalar registers they would spill
  const int s = blockIdx.x, tid = threadIdx.x;
  const int ri = sel[s];
  if (ri < 0) return;
  const long long lo = off[s], n = off[s + 1] - lo;
  const long long nz = (n + EQ_TILE - 1) / EQ_TILE - 1;             // the records: one per tile in front of the last
  if (nz < 1) return;
  const double* P6 = coef + (long long)ri * EQ_ROW + 32 + 6 * EQ_D * EQ_D;
  for (int i = tid; i < 6 * EQ_D * EQ_D; i += 64) PT[i] = P6[i];
  __syncthreads();
  double* rs = rec + (lo / EQ_TILE + s) * EQ_D;
  double c[EQ_D];                                                   // the state behind the batch before this one, in every lane
#pragma unroll
  for (int q = 0; q < EQ_D; ++q) c[q] = 0.0;
  for (long long b = 0; b < nz; b += 63) {                          // a batch: the carry in lane 0, then 63 tiles, one per lane
    const long long j = b + tid - 1;
    double z[EQ_D];
#pragma unroll
    for (int q = 0; q < EQ_D; ++q) z[q] = tid == 0 ? c[q] : j < nz ? rs[j * EQ_D + q] : 0.0;
#pragma nounroll
    for (int k = 0; k < 6; ++k) {                                   // inclusive scan: lane i > 0 ends with the true state behind tile b + i - 1
                                                                    // (not unrolled: the six matrices are read where they are used, not held)
      const int d = 1 << k;
      const double* Pd = PT + k * EQ_D * EQ_D;
      double u[EQ_D];
#pragma unroll
      for (int q = 0; q < EQ_D; ++q) u[q] = __shfl_up(z[q], d, 64);
      if (tid >= d) {
#pragma unroll
        for (int r = 0; r < EQ_D; ++r) {
          double a = z[r];
#pragma unroll
          for (int q = 0; q < EQ_D; ++q) a = fma(Pd[r * EQ_D + q], u[q], a);
          z[r] = a;
        }
      }
    }
    if (tid > 0 && j < nz) {
#pragma unroll
      for (int q = 0; q < EQ_D; ++q) rs[j * EQ_D + q] = z[q];
    }
#pragma unroll
    for (int q = 0; q < EQ_D; ++q) c[q] = __shfl(z[q], 63, 64);     // read only when another batch follows: then this one was full
  }
}

__global__ __launch_bounds__(64 * EQ_WAVES) void equalize_apply_k(const float* x, float* y, const long long* __restrict__ off,
                                                                  const int32_t* __restrict__ sel, const double* __restrict__ coef,
                                                                  const double* __restrict__ rec) {
  __shared__ float tile[EQ_WAVES * EQ_TILE];
  const int s = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const long long lo = off[s], n = off[s + 1] - lo;
  const long long nt = (n + EQ_TILE - 1) / EQ_TILE;
  if ((long long)blockIdx.x * EQ_WAVES >= nt) return;               // the whole workgroup: nothing waits at a barrier
  const long long j = (long long)blockIdx.x * EQ_WAVES + w;         // this wave's tile of the segment
  const long long t0 = j * EQ_TILE;
  const int tl = j < nt ? (int)min((long long)EQ_TILE, n - t0) : 0; // 0: no such tile
  const int ri = sel[s];
  const float* xs = x + lo + t0;
  float* ys = y + lo + t0;
  if (ri < 0) {                                                     // copied through (the whole workgroup)
    if (x != y)
      for (int i = l; i < tl; i += 64) ys[i] = xs[i];
    return;
  }
  float* tw = tile + w * EQ_TILE;
  for (int i = l; i < tl; i += 64) tw[i] = xs[i];
  __syncthreads();
  const double* R = coef + (long long)ri * EQ_ROW;
  const double* entry = tl > 0 && j > 0 ? rec + (lo / EQ_TILE + s + j - 1) * EQ_D : nullptr;
  switch ((int)R[0]) {                                              // workgroup-uniform: the row is the segment's
    case 1: eq_apply<1>(R, tw, tl, l, entry); break;
    case 2: eq_apply<2>(R, tw, tl, l, entry); break;
    case 3: eq_apply<3>(R, tw, tl, l, entry); break;
    default: eq_apply<4>(R, tw, tl, l, entry); break;
  }
  __syncthreads();
  for (int i = l; i < tl; i += 64) ys[i] = tw[i];
}

hipError_t launch_equalize_ragged(const float* x, float* y, const long long* off, int n_seg, long long tiles_max, const int32_t* sel,
                                  const double* coef, double* rec, hipStream_t st) {
  if (n_seg <= 0 || tiles_max <= 0) return hipSuccess;
  hipError_t e;
  if (tiles_max > 1) {                                              // some segment has a tile in front of its last
    hipLaunchKernelGGL(equalize_state_k, dim3((unsigned)((tiles_max - 1 + EQ_WAVES - 1) / EQ_WAVES), (unsigned)n_seg), dim3(64 * EQ_WAVES), 0, st,
                       x, off, sel, coef, rec);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(equalize_scan_k, dim3((unsigned)n_seg), dim3(64), 0, st, off, sel, coef, rec);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(equalize_apply_k, dim3((unsigned)((tiles_max + EQ_WAVES - 1) / EQ_WAVES), (unsigned)n_seg), dim3(64 * EQ_WAVES), 0, st, x, y,
                     off, sel, coef, rec);
  return hipGetLastError();
}
