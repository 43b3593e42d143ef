// Pause control on the device (ctts_trim_pauses_ragged): packed float32 segments lose their edge silence and the middle of long inner
// pauses, in frames of F = fs / 100 samples (chattts_amd/pauses.py holds the definition and the host side).  The decision is integer
// arithmetic on frames, so the result equals the host definition bit for bit.  The output length depends on the samples, so the output
// offsets are computed here, on the device.  Four launches:
//  * pause_frames_k -- the only pass that reads the whole signal to decide anything.  A wave reads a span of PA_FPW frames with 16-byte
//    loads at the pack's own alignment (single samples at the span's ragged ends: packed offsets are no multiples of 4 behind the
//    resampler), every lane collects a bit per frame for !(|x| < thr) (a NaN makes a frame active), the wave ORs the masks and writes one
//    byte per frame.
//  * pause_plan_k -- one workgroup per segment walks the frames in chunks of 256: a reverse min-scan gives na(j), the first active frame
//    >= j (second pass, from the end; parked in mix[]), an inclusive max-scan gives pa(j), the last active frame <= j, every frame applies
//    the rules, and an exclusive sum-scan of the kept frames' sample counts gives dst[j], the frame's place in the segment's output (-1:
//    dropped).  mix[j] is the crossfade partner (-1: none).  The carries of the three scans stay in registers.  Nothing depends on
//    anything outside the segment.
//  * pause_offsets_k -- one workgroup, the exclusive scan of the segments' output lengths -> off_out [n_seg + 1] int64.
//  * pause_copy_k -- a wave per kept frame copies it to out + off_out[s] + dst[j] with the widest access both alignments allow (16, 8 or
//    4 bytes), or crossfades it with its partner: the fade table w_in[F] comes through LDS (w_out[i] = w_in[F - 1 - i]), products and sum
//    rounded separately (__fmul_rn / __fadd_rn: no fused multiply-add, so float32 NumPy reproduces it).
//
// A STREAM (ctts_trim_pauses_stream_step): the segment arrives in pushes and the kept frames leave as soon as the rules decide them
// (pauses.py: schedule, state).  A slot's carry holds the frames that wait, two ranges of the current run and a function of (mode, frames
// seen, pa) alone, and the samples of the incomplete frame; a step reads buffer `phase` and writes the other.  Three launches:
//  * pause_stream_act_k  -- a wave per newly completed frame of (partial ++ push): one wave-wide reduction of !(|x| < thr) per frame.
//  * pause_stream_walk_k -- a wave per stream walks its new frames in order, 64 activity bits per ballot, every lane holding the same few
//    integers of state; what a frame decides goes to the stream's copy list, ranges of frames written by the lanes side by side.  Behind
//    the frames it lists the next carry, writes the slot's state and record, and reports (samples out, frames held, entries).
//  * pause_stream_copy_k -- a wave per entry of the copy lists, grid-wide: a frame to the chunk or to the new carry, sample by sample
//    across the lanes (F = 110, 220 put no frame start on 16 bytes, and a frame may begin in the carry and end in the push), or the
//    crossfade of two frames by pa_fade.
#include "common.hpp"
#include "kernels.hpp"

struct PauseRow {       // PA_ROW int32 (pauses.tables)
  int32_t F, pad, lead, tail, P;
  float thr;
  int32_t fade, reserved;
};
static_assert(sizeof(PauseRow) == PA_ROW * 4, "a pause row is PA_ROW int32");

#define PA_NONE 0x7fffffff     // na(j) when no active frame follows

__global__ __launch_bounds__(256) void pause_frames_k(const float* __restrict__ x, const long long* __restrict__ off,
                                                      const long long* __restrict__ fbase, const PauseRow* __restrict__ rows,
                                                      uint8_t* __restrict__ act) {
  const int s = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const PauseRow r = rows[s];
  if (r.P == 0) return;                                           // copied through: nobody reads its activity
  const long long lo = off[s], n = off[s + 1] - lo, fb = fbase[s], nF = fbase[s + 1] - fb;
  const long long j0 = ((long long)blockIdx.x * 4 + w) * PA_FPW;  // this wave's first frame
  if (j0 >= nF) return;
  const int F = r.F;
  const float thr = r.thr;
  const long long a = lo + j0 * F, b = lo + min(n, (j0 + PA_FPW) * F);   // the span, in samples of the pack
  unsigned m = 0;
  for (long long p = (a & ~3ll) + 4 * l; p < b; p += 256) {
    if (p >= a && p + 4 <= b) {
      const float4 v = *reinterpret_cast<const float4*>(x + p);
      const int rel = (int)(p - a), f = rel / F, q = rel - f * F; // the first sample's frame and its place in it; F >= 80: two frames at most
      if (!(fabsf(v.x) < thr)) m |= 1u << f;
      if (!(fabsf(v.y) < thr)) m |= 1u << (f + (q + 1 >= F));
      if (!(fabsf(v.z) < thr)) m |= 1u << (f + (q + 2 >= F));
      if (!(fabsf(v.w) < thr)) m |= 1u << (f + (q + 3 >= F));
    } else {
      for (long long i = max(p, a); i < min(p + 4, b); ++i)
        if (!(fabsf(x[i]) < thr)) m |= 1u << ((int)(i - a) / F);
    }
  }
  for (int d = 32; d >= 1; d >>= 1) m |= __shfl_xor(m, d, 64);
  if (l < PA_FPW && j0 + l < nF) act[fb + j0 + l] = (uint8_t)((m >> l) & 1u);
}

// inclusive scan of v over the 256 threads under op (associative, identity id); total: the block's result, the same in every thread
template <class T, class Op>
__device__ __forceinline__ T pa_block_scan(T v, T* sh, int tid, Op op, T id, T& total) {
  const int l = tid & 63, w = tid >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const T u = __shfl_up(v, d, 64);
    if (l >= d) v = op(u, v);
  }
  if (l == 63) sh[w] = v;
  __syncthreads();
  T pre = id;
  total = id;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const T t = sh[i];
    if (i < w) pre = op(pre, t);
    total = op(total, t);
  }
  __syncthreads();                                                // sh is free for the next scan
  return op(pre, v);
}

__global__ __launch_bounds__(256) void pause_plan_k(const long long* __restrict__ off, const long long* __restrict__ fbase,
                                                    const PauseRow* __restrict__ rows, const uint8_t* __restrict__ act,
                                                    int32_t* __restrict__ dst, int32_t* mix, int32_t* __restrict__ seg_len,
                                                    int32_t* __restrict__ records) {
  __shared__ int sh[4];
  __shared__ int rec[PA_REC];
  const int s = blockIdx.x, tid = threadIdx.x;
  const PauseRow r = rows[s];
  const long long n = off[s + 1] - off[s], fb = fbase[s];
  const int nF = (int)(fbase[s + 1] - fb), F = r.F;
  const uint8_t* as = act + fb;
  int32_t* ds = dst + fb;
  int32_t* ms = mix + fb;
  if (r.P == 0) {                                                 // the identity plan
    for (int j = tid; j < nF; j += 256) { ds[j] = j * F; ms[j] = -1; }
    if (tid == 0) {
      seg_len[s] = (int32_t)n;
      int32_t* o = records + (long long)s * PA_REC;
      o[0] = nF; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0; o[7] = (int32_t)n;
    }
    return;
  }
  if (tid < PA_REC) rec[tid] = 0;
  // na(j), from the end: thread t of a chunk takes frame hi - 1 - t, so an inclusive min-scan over t covers the frames >= j of the chunk
  int carry_na = PA_NONE;
  for (int hi = nF; hi > 0; hi -= 256) {
    const int j = hi - 1 - tid;
    int tot;
    const int inc = pa_block_scan<int>(j >= 0 && as[j] ? j : PA_NONE, sh, tid, [](int a, int b) { return min(a, b); }, PA_NONE, tot);
    if (j >= 0) ms[j] = min(inc, carry_na);
    carry_na = min(carry_na, tot);
  }
  __syncthreads();                                                // na is read by other threads than wrote it; rec[] is zero
  const int pad = r.pad, lead = r.lead, tail = r.tail, P = r.P, h = (P + 1) >> 1, t = P - h;
  int carry_pa = -1, carry_sum = 0;
  int c_act = 0, c_speech = 0, c_lead = 0, c_tail = 0, c_runs = 0, c_inner = 0;
  for (int base = 0; base < nF; base += 256) {
    const int j = base + tid;
    const bool in = j < nF;
    const bool a = in && as[j];
    int tot;
    const int pa = max(carry_pa, pa_block_scan<int>(a ? j : -1, sh, tid, [](int a, int b) { return max(a, b); }, -1, tot));
    carry_pa = max(carry_pa, tot);
    bool keep = false;
    int partner = -1;
    if (in) {
      const int na = ms[j];
      const bool has_pa = pa >= 0, has_na = na != PA_NONE;
      c_act += a;
      if ((has_pa && j - pa <= pad) || (has_na && na - j <= pad)) {
        keep = true;
        ++c_speech;
      } else {
        const int r0 = has_pa ? pa + pad + 1 : 0, r1 = has_na ? na - pad : nF, R = r1 - r0, k = j - r0;
        if (!has_pa && !has_na) {                                 // no active frame at all: the output is never empty
          keep = k < max(1, lead + tail);
          c_tail += !keep;
        } else if (!has_pa) {
          keep = k >= R - lead;
          c_lead += !keep;
        } else if (!has_na) {
          keep = k < tail;
          c_tail += !keep;
        } else if (R <= P) {
          keep = true;
        } else {
          keep = k < h || k >= R - t;
          c_inner += !keep;
          c_runs += k == 0;
          if (k == h - 1) partner = r1 - t - 1;
        }
      }
    }
    const int len = !keep ? 0 : j == nF - 1 ? (int)(n - (long long)j * F) : F;
    const int inc = pa_block_scan<int>(len, sh, tid, [](int a, int b) { return a + b; }, 0, tot);
    if (in) {
      ds[j] = keep ? carry_sum + inc - len : -1;
      ms[j] = partner;
    }
    carry_sum += tot;
  }
  atomicAdd(&rec[1], c_act); atomicAdd(&rec[2], c_speech); atomicAdd(&rec[3], c_lead); atomicAdd(&rec[4], c_tail);
  atomicAdd(&rec[5], c_runs); atomicAdd(&rec[6], c_inner);
  __syncthreads();
  if (tid == 0) { rec[0] = nF; rec[7] = carry_sum; seg_len[s] = carry_sum; }
  __syncthreads();
  if (tid < PA_REC) records[(long long)s * PA_REC + tid] = rec[tid];
}

__global__ __launch_bounds__(256) void pause_offsets_k(const int32_t* __restrict__ seg_len, long long* __restrict__ off_out, int n_seg) {
  __shared__ long long sh[4];
  const int tid = threadIdx.x;
  long long carry = 0;
  if (tid == 0) off_out[0] = 0;
  for (int base = 0; base < n_seg; base += 256) {
    const int s = base + tid;
    long long tot;
    const long long inc = pa_block_scan<long long>(s < n_seg ? (long long)seg_len[s] : 0ll, sh, tid, [](long long a, long long b) { return a + b; }, 0ll, tot);
    if (s < n_seg) off_out[s + 1] = carry + inc;
    carry += tot;
  }
}

// one sample of the crossfade: two products and their sum, each rounded to nearest on its own.  __fmul_rn / __fadd_rn are plain operators
// in the HIP headers and carry the translation unit's permission to contract, so a sum of two of them still fuses into a multiply-add
// (loudness_scale_k has a product alone, which cannot).  Here the operators are written out with contraction switched off: the
// instructions are v_mul_f32 / v_add_f32 (or their packed forms), never a v_fma
__device__ __forceinline__ float pa_fade(float w_out, float a, float w_in, float b) {
#pragma clang fp contract(off)
  const float p = w_out * a;
  const float q = w_in * b;
  return p + q;
}

// one frame of len samples, x[0 ..) -> y[0 ..), by the wave: V floats per access where xi and yi (the two positions in their 16-byte
// aligned buffers) are congruent mod V, single samples in front of the first aligned position and behind the last whole vector
template <int V, class T>
__device__ __forceinline__ void pa_copy_frame(const float* x, float* y, long long yi, int len, int l) {
  const int head = min(len, (int)((V - (yi & (V - 1))) & (V - 1))), nv = (len - head) / V;
  if (l < head) y[l] = x[l];
  for (int v = l; v < nv; v += 64) *reinterpret_cast<T*>(y + head + v * V) = *reinterpret_cast<const T*>(x + head + v * V);
  const int i = head + nv * V + l;
  if (i < len) y[i] = x[i];
}

__global__ __launch_bounds__(256) void pause_copy_k(const float* __restrict__ x, float* __restrict__ y, const long long* __restrict__ off,
                                                    const long long* __restrict__ fbase, const PauseRow* __restrict__ rows,
                                                    const long long* __restrict__ off_out, const int32_t* __restrict__ dst,
                                                    const int32_t* __restrict__ mix, const float* __restrict__ fade) {
  __shared__ float win[PA_FMAX];
  const int s = blockIdx.y, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const long long fb = fbase[s];
  const int nF = (int)(fbase[s + 1] - fb), jb = blockIdx.x * PA_FPB;
  if (jb >= nF) return;                                           // the whole workgroup
  const PauseRow r = rows[s];
  const int F = r.F;
  const long long lo = off[s], n = off[s + 1] - lo, ob = off_out[s];
  const int32_t* ds = dst + fb;
  const int32_t* ms = mix + fb;
  const int fades = tid < PA_FPB && jb + tid < nF && ms[jb + tid] >= 0;
  if (__syncthreads_or(fades)) {                                  // a crossfade among this workgroup's frames: the table goes to LDS
    for (int i = tid; i < F; i += 256) win[i] = fade[r.fade + i];
    __syncthreads();
  }
  for (int q = 0; q < PA_FPB / 4; ++q) {
    const int j = jb + w * (PA_FPB / 4) + q;
    if (j >= nF) break;
    const int d = ds[j];
    if (d < 0) continue;
    const long long xi = lo + (long long)j * F, yi = ob + d;
    const int len = j == nF - 1 ? (int)(n - (long long)j * F) : F;
    const int m = ms[j];
    if (m >= 0) {                                                 // both frames are interior: F samples each
      const float* xa = x + xi;
      const float* xb = x + lo + (long long)m * F;
      for (int i = l; i < F; i += 64) y[yi + i] = pa_fade(win[F - 1 - i], xa[i], win[i], xb[i]);
    } else if (((xi - yi) & 3) == 0) {
      pa_copy_frame<4, float4>(x + xi, y + yi, yi, len, l);
    } else if (((xi - yi) & 1) == 0) {
      pa_copy_frame<2, float2>(x + xi, y + yi, yi, len, l);
    } else {
      for (int i = l; i < len; i += 64) y[yi + i] = x[xi + i];
    }
  }
}

// ---- streams --------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(PaStream) == 96 && sizeof(PaCopy) == 16 && PA_STATE >= 3 + PA_REC, "pause stream tables");

struct PaConsts {
  int P, lead, tail, pad, h, t, k0, A1, A2, H, L;
};
__device__ __forceinline__ PaConsts pa_consts(const PaStream& D) {
  PaConsts c;
  c.P = D.P; c.lead = D.lead; c.tail = D.tail; c.pad = D.pad;
  c.h = (c.P + 1) >> 1; c.t = c.P - c.h; c.k0 = min(c.h - 1, c.tail);
  c.A1 = max(1, c.lead + c.tail); c.A2 = c.lead + c.pad; c.H = max(c.h, c.tail); c.L = c.t + 1 + c.pad;
  return c;
}
// pauses.stream_held: the run starts at frame r0; its frames k in [lo, a) and [b, m) wait, in this order
struct PaHeld {
  int r0, lo, a, b, m;
};
__device__ __forceinline__ PaHeld pa_held(const PaConsts& c, int mode, int nfr, int pa) {
  PaHeld o;
  if (mode == 0) {
    o.r0 = 0; o.lo = 0; o.m = nfr; o.a = min(o.m, c.A1); o.b = max(o.a, o.m - c.A2);
    return o;
  }
  o.r0 = pa + c.pad + 1; o.lo = c.k0; o.m = max(nfr - o.r0, c.k0);
  if (o.m - c.pad <= c.P) { o.a = o.m; o.b = o.m; }
  else { o.a = min(o.m, c.H); o.b = max(o.a, o.m - c.L); }
  return o;
}
// sample i of the frame a copy-list code names: a frame of the old carry, or frame q of (partial ++ push)
struct PaSrc {
  const float* cold;   // the slot's old carry buffer
  const float* xin;    // the push
  int F, pn;           // pn: samples of the partial frame in the old carry
};
__device__ __forceinline__ float pa_read(const PaSrc& S, int code, int i) {
  if (code < PA_SCAP) return S.cold[code * S.F + i];
  const long long p = (long long)(code - PA_SCAP) * S.F + i;
  return p < S.pn ? S.cold[PA_SCAP * PA_FMAX + p] : S.xin[p - S.pn];
}

__global__ __launch_bounds__(256) void pause_stream_act_k(const float* __restrict__ x, const PaStream* __restrict__ tab,
                                                          const float* __restrict__ carry, uint8_t* __restrict__ act) {
  const PaStream& D = tab[blockIdx.y];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, F = D.F, pn = (int)(D.pos % F);
  const long long avail = pn + D.n_in, nf = avail / F + (D.fin && avail % F ? 1 : 0), q = (long long)blockIdx.x * 4 + w;
  if (q >= nf) return;                                            // the whole wave
  const float* part = carry + ((long long)D.slot * 2 + D.phase) * PA_SCARRY + PA_SCAP * PA_FMAX;
  const float* xin = x + D.in_off;
  const long long a = q * F, b = min(avail, a + F);
  const float thr = D.thr;
  int hit = 0;
  for (long long p = a + l; p < b; p += 64) {
    const float v = p < pn ? part[p] : xin[p - pn];
    hit |= !(fabsf(v) < thr);
  }
  hit = __any(hit);
  if (l == 0) act[D.fr_off + q] = (uint8_t)(hit != 0);
}

__global__ __launch_bounds__(64) void pause_stream_walk_k(const PaStream* __restrict__ tab, const uint8_t* __restrict__ act,
                                                          int32_t* __restrict__ state, PaCopy* __restrict__ list, int32_t* __restrict__ res) {
  const PaStream& D = tab[blockIdx.x];
  const int l = threadIdx.x, F = D.F, pn = (int)(D.pos % F);
  const PaConsts c = pa_consts(D);
  const long long avail = pn + D.n_in;
  const int nfull = (int)(avail / F), plen = (int)(avail - (long long)nfull * F), nf = nfull + (D.fin && plen ? 1 : 0);
  int32_t* st = state + (long long)D.slot * PA_STATE;
  int mode = 0, nfr = 0, pa = 0, rec[PA_REC] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (D.pos != 0) {                                               // at pos == 0 the slot is fresh by its descriptor alone
    mode = st[0]; nfr = st[1]; pa = st[2];
#pragma unroll
    for (int i = 0; i < PA_REC; ++i) rec[i] = st[3 + i];
  }
  const PaHeld o = pa_held(c, mode, nfr, pa);
  const int nfr0 = nfr, jpart = D.fin && plen ? nfr0 + nfull : -1;
  auto src = [&](int j) {
    if (j >= nfr0) return PA_SCAP + (j - nfr0);
    const int k = j - o.r0;
    return k < o.a ? k - o.lo : (o.a - o.lo) + (k - o.b);
  };
  PaCopy* L = list + D.list_off;
  int ne = 0, n_out = 0;
  auto emit = [&](int j0, int j1) {                               // frames [j0, j1), copied: an entry per lane
    const int cnt = j1 - j0;
    if (cnt <= 0) return;
    for (int i = l; i < cnt; i += 64) {
      PaCopy e;
      e.src = src(j0 + i); e.mix = -1; e.dst = n_out + i * F; e.len = j0 + i == jpart ? plen : F;
      L[ne + i] = e;
    }
    n_out += cnt * F - (jpart >= j0 && jpart < j1 ? F - plen : 0);
    ne += cnt;
  };
  const uint8_t* A = act + D.fr_off;
  for (int base = 0; base < nf; base += 64) {
    const unsigned long long bits = __ballot(base + l < nf && A[base + l] != 0);
    const int top = min(64, nf - base);
    for (int q = 0; q < top; ++q) {
      const int j = nfr++;
      if ((bits >> q) & 1ull) {
        ++rec[1];
        if (mode == 0) {
          const int first = max(0, j - c.pad - c.lead);
          emit(first, j);
          rec[3] += first;
          rec[2] += min(j, c.pad) + 1;
          mode = 1;
        } else {
          const int r0 = pa + c.pad + 1, m = j - r0, R = m - c.pad;
          rec[2] += min(j - pa - 1, 2 * c.pad) + 1;
          if (R <= c.P) {
            emit(r0 + c.k0, r0 + m);
          } else {
            emit(r0 + c.k0, r0 + c.h - 1);
            if (l == 0) {                                         // both frames are full: they lie in front of an active frame
              PaCopy e;
              e.src = src(r0 + c.h - 1); e.mix = src(r0 + R - c.t - 1); e.dst = n_out; e.len = F;
              L[ne] = e;
            }
            ++ne;
            n_out += F;
            emit(r0 + R - c.t, r0 + m);
            ++rec[5];
            rec[6] += R - c.P;
          }
        }
        emit(j, j + 1);
        pa = j;
      } else if (mode == 1 && (j - pa <= c.pad || j - pa - c.pad - 1 < c.k0)) {
        emit(j, j + 1);
      }
    }
  }
  int held = 0;
  if (D.fin) {
    if (mode == 0) {
      const int keep = min(nfr, c.A1);
      emit(0, keep);
      rec[4] += nfr - keep;
    } else {
      const int r0 = pa + c.pad + 1, R = nfr - r0;
      rec[2] += min(nfr - 1 - pa, c.pad);
      if (R > 0) {
        emit(r0 + c.k0, r0 + min(c.tail, R));
        rec[4] += max(0, R - c.tail);
      }
    }
    rec[0] = nfr;
  } else {                                                        // the next carry: the frames that wait, then the partial frame
    const PaHeld n = pa_held(c, mode, nfr, pa);
    const int n1 = n.a - n.lo;
    held = n1 + (n.m - n.b);
    for (int i = l; i < held; i += 64) {
      PaCopy e;
      e.src = src(n.r0 + (i < n1 ? n.lo + i : n.b + (i - n1))); e.mix = -1; e.dst = -1 - i * F; e.len = F;
      L[ne + i] = e;
    }
    ne += held;
    if (plen) {
      if (l == 0) {
        PaCopy e;
        e.src = PA_SCAP + nfull; e.mix = -1; e.dst = -1 - PA_SCAP * PA_FMAX; e.len = plen;
        L[ne] = e;
      }
      ++ne;
    }
  }
  rec[7] += n_out;
  if (l == 0) {
    st[0] = mode; st[1] = nfr; st[2] = pa;
#pragma unroll
    for (int i = 0; i < PA_REC; ++i) st[3 + i] = rec[i];
    int32_t* r = res + (long long)blockIdx.x * PA_RES;
    r[0] = n_out; r[1] = held; r[2] = ne; r[3] = 0;
  }
}

__global__ __launch_bounds__(256) void pause_stream_copy_k(const float* __restrict__ x, const PaStream* __restrict__ tab,
                                                           const PaCopy* __restrict__ list, const int32_t* __restrict__ res,
                                                           float* __restrict__ y, float* carry, const float* __restrict__ fade) {
  const PaStream& D = tab[blockIdx.y];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const long long e = (long long)blockIdx.x * 4 + w;
  if (e >= res[(long long)blockIdx.y * PA_RES + 2]) return;       // the whole wave
  const PaCopy cp = list[D.list_off + e];
  PaSrc S;
  S.F = D.F; S.pn = (int)(D.pos % D.F);
  S.cold = carry + ((long long)D.slot * 2 + D.phase) * PA_SCARRY;
  S.xin = x + D.in_off;
  float* dst = cp.dst >= 0 ? y + D.out_off + cp.dst : carry + ((long long)D.slot * 2 + (D.phase ^ 1)) * PA_SCARRY + (-1 - cp.dst);
  if (cp.mix >= 0) {
    const float* win = fade + D.fade;
    for (int i = l; i < S.F; i += 64) dst[i] = pa_fade(win[S.F - 1 - i], pa_read(S, cp.src, i), win[i], pa_read(S, cp.mix, i));
  } else {
    for (int i = l; i < cp.len; i += 64) dst[i] = pa_read(S, cp.src, i);
  }
}

hipError_t launch_trim_pauses_stream(const float* x, const PaStream* tab, int n_streams, long long nf_max, long long list_max, long long frames,
                                     float* y, float* carry, int32_t* state, const float* fade, int32_t* res, void* scratch, hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  uint8_t* act = (uint8_t*)scratch;
  PaCopy* list = (PaCopy*)((char*)scratch + pause_r16((size_t)frames));
  hipError_t e;
  if (nf_max > 0) {
    hipLaunchKernelGGL(pause_stream_act_k, dim3((unsigned)((nf_max + 3) / 4), (unsigned)n_streams), dim3(256), 0, st, x, tab, (const float*)carry, act);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pause_stream_walk_k, dim3((unsigned)n_streams), dim3(64), 0, st, tab, (const uint8_t*)act, state, list, res);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (list_max > 0)
    hipLaunchKernelGGL(pause_stream_copy_k, dim3((unsigned)((list_max + 3) / 4), (unsigned)n_streams), dim3(256), 0, st, x, tab,
                       (const PaCopy*)list, (const int32_t*)res, y, carry, fade);
  return hipGetLastError();
}

hipError_t launch_trim_pauses_ragged(const float* x, float* y, const long long* off, const long long* fbase, const int32_t* rows, int n_seg,
                                     long long frames_max, long long frames, const float* fade, long long* off_out, int32_t* records,
                                     void* scratch, hipStream_t st) {
  if (n_seg <= 0 || frames_max <= 0 || frames <= 0) return hipSuccess;
  char* sp = (char*)scratch;
  int32_t* dst = (int32_t*)sp;
  sp += pause_r16((size_t)frames * 4);
  int32_t* mix = (int32_t*)sp;
  sp += pause_r16((size_t)frames * 4);
  uint8_t* act = (uint8_t*)sp;
  sp += pause_r16((size_t)frames);
  int32_t* seg_len = (int32_t*)sp;
  const PauseRow* rw = (const PauseRow*)rows;
  const dim3 g1((unsigned)((frames_max + 4 * PA_FPW - 1) / (4 * PA_FPW)), (unsigned)n_seg);
  hipLaunchKernelGGL(pause_frames_k, g1, dim3(256), 0, st, x, off, fbase, rw, act);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pause_plan_k, dim3((unsigned)n_seg), dim3(256), 0, st, off, fbase, rw, (const uint8_t*)act, dst, mix, seg_len, records);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pause_offsets_k, dim3(1), dim3(256), 0, st, (const int32_t*)seg_len, off_out, n_seg);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 g4((unsigned)((frames_max + PA_FPB - 1) / PA_FPB), (unsigned)n_seg);
  hipLaunchKernelGGL(pause_copy_k, g4, dim3(256), 0, st, x, y, off, fbase, rw, (const long long*)off_out, (const int32_t*)dst,
                     (const int32_t*)mix, fade);
  return hipGetLastError();
}
