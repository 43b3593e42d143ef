// Micro-benchmarks of the fixed cost of a short dependent kernel on MI355X: the kernel-argument fetch at its head (parts "size" and
// "preload") and the write-back of its results at its end (part "publish").  Own main, no Python.
//
// "size"    (round 3: growing DecGemmArgs by 32 bytes made the 5 us o_proj launch 1 us slower.)  Does the SIZE of a by-value
//           argument struct matter?  A chain of 104 graph-captured launches; each kernel reads a pointer from the FIRST or the LAST
//           8 bytes of an N-byte struct, loads what the previous kernel wrote, writes one value.
//
// "preload" Does the scalar load of the kernel-argument segment, which nothing in the body can be addressed before, cost time in a
//           step-like chain, and does kernarg preload (leading arguments placed in user SGPRs at dispatch) take it away?  The same
//           104-launch captured chain, every hop with a decode-projection-like body: each of 192 workgroups requests 24 KB of cold
//           "weights" (non-temporal, as tools/overlap_probe.hip), reads the live-row count through a pointer (the second dependent
//           scalar load of the real kernels), then the value a workgroup of the previous hop wrote, and writes its own.
//             struct   all arguments in one by-value struct: preload length 0, the body starts with s_load of the segment
//             preload  the same values as leading plain parameters: with -mllvm -amdgpu-kernarg-preload-count=16 they arrive in SGPRs
//           each in two cache states:
//             hot      the graph is the chain alone, replayed back to back
//             cold     a kernel node that streams 512 MB with non-temporal loads runs ahead of the chain in the same graph, so every
//                      argument segment was last touched half a gigabyte of traffic ago; the stream node alone is timed in the same
//                      repeat and subtracted
//           Four cells, three repeats each, us per launch.  The final values of the chain are checked (one increment per hop).
//           Read the preload length the compiler granted with:  hipcc ... --cuda-device-only -S, .amdhsa_user_sgpr_kernarg_preload_length
//
// "publish" Does it pay to store a launch's results write-through (sc1), so that the release at the end of the launch finds the L2 of
//           each XCD clean, instead of plain stores whose dirty lines that release has to write back?  The "preload" chain (104
//           captured launches, 24 KB of cold weights per workgroup, the previous hop's value read from a workgroup on another XCD),
//           but every workgroup stores 4 KB (16 bytes per lane), 192 and 768 workgroups = 0.79 and 3.1 MB dirtied per launch:
//             plain    global_store_dwordx4
//             sc1      the same store through a buffer resource with the write-through bit (aux 16)
//           alternating, three repeats each, us per launch; the chain's values are checked.
//
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 tools/kernarg_probe.hip -o /tmp/kernarg_probe
//   /tmp/kernarg_probe [size|preload|publish]        (default: size and preload)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

// ---- part "size" -------------------------------------------------------------------------------------------------------------
template <int N> struct Args { const float* first; char pad[N - 24]; float* out; const float* last; };
template <> struct Args<24> { const float* first; float* out; const float* last; };

template <int N, bool LAST>
__global__ void k_hop(Args<N> a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const float* in = LAST ? a.last : a.first;
  a.out[i] = in[(i + 4096) & 16383] + 1.0f;
}

template <int N, bool LAST>
static int run(float* b0, float* b1, hipStream_t st, int grid) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipGraph_t g; hipGraphExec_t ge;
  CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < 104; ++i) {
    Args<N> a; memset(&a, 0, sizeof(a));
    a.first = a.last = (i & 1) ? b1 : b0; a.out = (i & 1) ? b0 : b1;
    hipLaunchKernelGGL((k_hop<N, LAST>), dim3(grid), dim3(256), 0, st, a);
  }
  CK(hipStreamEndCapture(st, &g));
  CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  for (int w = 0; w < 3; ++w) CK(hipGraphLaunch(ge, st));
  CK(hipStreamSynchronize(st));
  CK(hipEventRecord(e0, st));
  for (int rep = 0; rep < 30; ++rep) CK(hipGraphLaunch(ge, st));
  CK(hipEventRecord(e1, st));
  CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  printf("args %4zu bytes, pointer read from the %s field, grid %3d: %.3f us per kernel\n", sizeof(Args<N>), LAST ? "LAST " : "FIRST", grid, ms * 1e3 / (30.0 * 104));
  CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
  return 0;
}

static int part_size(hipStream_t st) {
  float *b0, *b1;
  CK(hipMalloc(&b0, 65536 * 4)); CK(hipMalloc(&b1, 65536 * 4)); CK(hipMemset(b0, 0, 65536 * 4)); CK(hipMemset(b1, 0, 65536 * 4));
  for (int grid : {64, 192}) {
#define R(N) if (run<N, false>(b0, b1, st, grid)) return 1; if (run<N, true>(b0, b1, st, grid)) return 1;
    R(24) R(64) R(128) R(192) R(224) R(256) R(288) R(320) R(512) R(1024)
#undef R
  }
  CK(hipFree(b0)); CK(hipFree(b1));
  return 0;
}

// ---- part "preload" ----------------------------------------------------------------------------------------------------------
static const int CHAIN = 104, N_WG = 192, REPLAYS = 20, REPEATS = 3;
static const size_t HOP_W = (size_t)N_WG * 24576;              // weight bytes of one hop
static const size_t FLUSH_BYTES = (size_t)512 << 20;           // streamed ahead of the chain in the cold state
static const int FLUSH_WG = 1024;

typedef unsigned u4 __attribute__((ext_vector_type(4)));

struct HopArgs {        // what a decode projection's struct holds, in the order its body first needs it
  const u4* w;          // this hop's weights: N_WG * 24 KB
  const int* n_live;    // live-row count on the device (1 here): gates the activation load as *n_active does
  const unsigned* in;   // the previous hop's output
  unsigned* out;
  unsigned n_elem;      // elements of in / out (N_WG * 256)
};

__device__ __forceinline__ void hop_body(const u4* w, const int* n_live, const unsigned* in, unsigned* out, unsigned n_elem) {
  const int tid = threadIdx.x, wg = blockIdx.x;
  u4 wv[6];
  const u4* wp = w + (size_t)wg * 1536 + tid;
#pragma unroll
  for (int j = 0; j < 6; ++j) wv[j] = __builtin_nontemporal_load(wp + j * 256);   // requested at kernel entry, as gemm_dec32x_k does
  __builtin_amdgcn_sched_barrier(0);                          // the weights are on their way before the live-row count is asked for
  const unsigned live = (unsigned)*n_live;                     // 1; part of the address, so that no branch lets hipcc sink the weight loads
  const unsigned i = (unsigned)wg * 256u + (unsigned)tid;
  const unsigned x = in[(i + live * 19u * 256u) % n_elem];     // a workgroup 19 further on: another XCD
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) s ^= wv[j].x ^ wv[j].y ^ wv[j].z ^ wv[j].w;   // the weights are zeros: s == 0
  out[i] = x + 1u + s;
}

extern "C" __global__ __launch_bounds__(256) void k_hop_struct(HopArgs a) { hop_body(a.w, a.n_live, a.in, a.out, a.n_elem); }
extern "C" __global__ __launch_bounds__(256) void k_hop_preload(const u4* w, const int* n_live, const unsigned* in, unsigned* out, unsigned n_elem) {
  hop_body(w, n_live, in, out, n_elem);
}

// streams n vectors (16 bytes each) once with non-temporal loads; the sum keeps the loads alive
extern "C" __global__ __launch_bounds__(256) void k_flush(const u4* p, size_t n, unsigned* sink) {
  unsigned s = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const u4 v = __builtin_nontemporal_load(p + i);
    s ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  sink[blockIdx.x * 256 + threadIdx.x] = s;
}

struct PBufs { u4 *w, *flush; unsigned *b0, *b1, *sink; int* n_live; };

// graph: [flush node] + [chain of 104 hops]; either part may be left out
static int build_graph(const PBufs& b, hipStream_t st, bool flush, int variant /* 0 struct, 1 preload, -1 no chain */, hipGraphExec_t* ge) {
  hipGraph_t g;
  CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  if (flush) hipLaunchKernelGGL(k_flush, dim3(FLUSH_WG), dim3(256), 0, st, (const u4*)b.flush, FLUSH_BYTES / 16, b.sink);
  for (int i = 0; variant >= 0 && i < CHAIN; ++i) {
    HopArgs a;
    a.w = (const u4*)((const char*)b.w + (size_t)i * HOP_W);
    a.n_live = b.n_live;
    a.in = (i & 1) ? b.b1 : b.b0; a.out = (i & 1) ? b.b0 : b.b1;
    a.n_elem = (unsigned)N_WG * 256u;
    if (variant == 0) hipLaunchKernelGGL(k_hop_struct, dim3(N_WG), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_hop_preload, dim3(N_WG), dim3(256), 0, st, a.w, a.n_live, a.in, a.out, a.n_elem);
  }
  CK(hipStreamEndCapture(st, &g));
  CK(hipGraphInstantiate(ge, g, nullptr, nullptr, 0));
  CK(hipGraphDestroy(g));
  return 0;
}

static int time_graph(hipGraphExec_t ge, hipStream_t st, hipEvent_t e0, hipEvent_t e1, double* us_per_replay) {
  CK(hipGraphLaunch(ge, st));   // one untimed replay: whatever ran before this cell is out of the picture
  CK(hipEventRecord(e0, st));
  for (int r = 0; r < REPLAYS; ++r) CK(hipGraphLaunch(ge, st));
  CK(hipEventRecord(e1, st));
  CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  *us_per_replay = ms * 1e3 / REPLAYS;
  return 0;
}

static int part_preload(hipStream_t st) {
  PBufs b;
  const size_t n_out = (size_t)N_WG * 256;
  CK(hipMalloc(&b.w, (size_t)CHAIN * HOP_W)); CK(hipMemset(b.w, 0, (size_t)CHAIN * HOP_W));
  CK(hipMalloc(&b.flush, FLUSH_BYTES)); CK(hipMemset(b.flush, 0, FLUSH_BYTES));
  CK(hipMalloc(&b.b0, n_out * 4)); CK(hipMalloc(&b.b1, n_out * 4)); CK(hipMemset(b.b0, 0, n_out * 4)); CK(hipMemset(b.b1, 0, n_out * 4));
  CK(hipMalloc(&b.sink, (size_t)FLUSH_WG * 256 * 4));
  const int one = 1;
  CK(hipMalloc(&b.n_live, 4)); CK(hipMemcpy(b.n_live, &one, 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipGraphExec_t hot[2], cold[2], flush_only;
  for (int v = 0; v < 2; ++v) { if (build_graph(b, st, false, v, &hot[v])) return 1; if (build_graph(b, st, true, v, &cold[v])) return 1; }
  if (build_graph(b, st, true, -1, &flush_only)) return 1;
  const char* vname[2] = {"struct ", "preload"};
  unsigned hops = 0;   // hops run so far: the value every element of b0 must hold at the end
  printf("chain of %d captured launches, %d workgroups x 24 KB of cold weights per hop, %d replays per figure; us per launch\n", CHAIN, N_WG, REPLAYS);
  for (int rep = 0; rep < REPEATS; ++rep) {
    double t_flush, t;
    if (time_graph(flush_only, st, e0, e1, &t_flush)) return 1;
    printf("repeat %d: flush node alone (512 MB non-temporal) %.1f us\n", rep, t_flush);
    for (int v = 0; v < 2; ++v) {
      if (time_graph(hot[v], st, e0, e1, &t)) return 1;
      hops += (unsigned)(REPLAYS + 1) * CHAIN;
      printf("repeat %d: %s hot   %.3f us per launch\n", rep, vname[v], t / CHAIN);
      if (time_graph(cold[v], st, e0, e1, &t)) return 1;
      hops += (unsigned)(REPLAYS + 1) * CHAIN;
      printf("repeat %d: %s cold  %.3f us per launch   (replay %.1f us - flush %.1f us)\n", rep, vname[v], (t - t_flush) / CHAIN, t, t_flush);
      fflush(stdout);
    }
  }
  std::vector<unsigned> h(n_out);
  CK(hipMemcpy(h.data(), b.b0, n_out * 4, hipMemcpyDeviceToHost));
  size_t bad = 0;
  for (unsigned x : h) bad += x != hops;
  printf("chain values %s (%zu of %zu wrong, expect %u, first %u)\n", bad ? "WRONG" : "ok", bad, h.size(), hops, h[0]);
  for (int v = 0; v < 2; ++v) { CK(hipGraphExecDestroy(hot[v])); CK(hipGraphExecDestroy(cold[v])); }
  CK(hipGraphExecDestroy(flush_only));
  return bad ? 1 : 0;
}

// ---- part "publish" ----------------------------------------------------------------------------------------------------------
static const int PUB_MAX_WG = 768;

// out / in: n_elem 16-byte vectors (one per thread of the grid); the vector's four words all hold the hop count
template <bool WT>
__global__ __launch_bounds__(256) void k_hop_pub(const u4* w, const int* n_live, const u4* in, u4* out, unsigned n_elem) {
  const int tid = threadIdx.x, wg = blockIdx.x;
  u4 wv[6];
  const u4* wp = w + (size_t)wg * 1536 + tid;
#pragma unroll
  for (int j = 0; j < 6; ++j) wv[j] = __builtin_nontemporal_load(wp + j * 256);
  __builtin_amdgcn_sched_barrier(0);
  const unsigned live = (unsigned)*n_live;
  const unsigned i = (unsigned)wg * 256u + (unsigned)tid;        // < n_elem: the grid is n_elem / 256 workgroups
  const u4 x = in[(i + live * 19u * 256u) % n_elem];
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) s ^= wv[j].x ^ wv[j].y ^ wv[j].z ^ wv[j].w;
  const u4 y = {x.x + 1u + s, x.y + 1u + s, x.z + 1u + s, x.w + 1u + s};
  if (WT) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, (int)(n_elem * 16u), 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(y, rs, (int)(i * 16u), 0, 16);   // aux 16 = sc1
  } else {
    out[i] = y;
  }
}

static int pub_graph(const PBufs& b, u4* o0, u4* o1, hipStream_t st, int n_wg, bool wt, hipGraphExec_t* ge) {
  hipGraph_t g;
  CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < CHAIN; ++i) {
    const u4* w = (const u4*)((const char*)b.w + (size_t)i * PUB_MAX_WG * 24576);
    const u4* in = (i & 1) ? o1 : o0; u4* out = (i & 1) ? o0 : o1;
    if (wt) hipLaunchKernelGGL(k_hop_pub<true>, dim3(n_wg), dim3(256), 0, st, w, (const int*)b.n_live, in, out, (unsigned)n_wg * 256u);
    else hipLaunchKernelGGL(k_hop_pub<false>, dim3(n_wg), dim3(256), 0, st, w, (const int*)b.n_live, in, out, (unsigned)n_wg * 256u);
  }
  CK(hipStreamEndCapture(st, &g));
  CK(hipGraphInstantiate(ge, g, nullptr, nullptr, 0));
  CK(hipGraphDestroy(g));
  return 0;
}

static int part_publish(hipStream_t st) {
  PBufs b;
  const size_t n_max = (size_t)PUB_MAX_WG * 256;
  u4 *o0, *o1;
  CK(hipMalloc(&b.w, (size_t)CHAIN * PUB_MAX_WG * 24576)); CK(hipMemset(b.w, 0, (size_t)CHAIN * PUB_MAX_WG * 24576));
  CK(hipMalloc(&o0, n_max * 16)); CK(hipMalloc(&o1, n_max * 16));
  const int one = 1;
  CK(hipMalloc(&b.n_live, 4)); CK(hipMemcpy(b.n_live, &one, 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  printf("chain of %d captured launches, 24 KB of cold weights and 4 KB of results per workgroup, %d replays per figure; us per launch\n", CHAIN, REPLAYS);
  int rc = 0;
  for (int n_wg : {192, 768}) {
    CK(hipMemset(o0, 0, n_max * 16)); CK(hipMemset(o1, 0, n_max * 16));
    hipGraphExec_t ge[2];
    for (int v = 0; v < 2; ++v) if (pub_graph(b, o0, o1, st, n_wg, v == 1, &ge[v])) return 1;
    unsigned hops = 0;
    double lo[2] = {1e30, 1e30}, hi[2] = {0, 0};
    for (int rep = 0; rep < REPEATS; ++rep)
      for (int v = 0; v < 2; ++v) {
        double t;
        if (time_graph(ge[v], st, e0, e1, &t)) return 1;
        hops += (unsigned)(REPLAYS + 1) * CHAIN;
        t /= CHAIN;
        lo[v] = t < lo[v] ? t : lo[v]; hi[v] = t > hi[v] ? t : hi[v];
        printf("%3d workgroups, repeat %d: %s %.3f us per launch\n", n_wg, rep, v ? "sc1  " : "plain", t);
        fflush(stdout);
      }
    std::vector<unsigned> h((size_t)n_wg * 256 * 4);
    CK(hipMemcpy(h.data(), o0, h.size() * 4, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (unsigned x : h) bad += x != hops;
    printf("%3d workgroups: plain %.3f-%.3f, sc1 %.3f-%.3f us per launch; chain values %s (%zu of %zu wrong, expect %u, first %u)\n", n_wg, lo[0], hi[0], lo[1],
           hi[1], bad ? "WRONG" : "ok", bad, h.size(), hops, h[0]);
    for (int v = 0; v < 2; ++v) CK(hipGraphExecDestroy(ge[v]));
    rc |= bad != 0;
  }
  return rc;
}

int main(int argc, char** argv) {
  const char* part = argc > 1 ? argv[1] : "both";
  hipStream_t st; CK(hipStreamCreate(&st));
  if (!strcmp(part, "publish")) return part_publish(st);
  if (strcmp(part, "preload") != 0 && part_size(st)) return 1;
  if (strcmp(part, "size") != 0 && part_preload(st)) return 1;
  return 0;
}
