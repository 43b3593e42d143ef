// extern "C" boundary of libchattts_amd.so (declared in include/chattts_amd.h) and the launch
// sequences of the GPT step / DVAE / Vocos.  No device allocation, no device synchronisation.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>

#include "../../include/chattts_amd.h"
#include "kernels.hpp"

static thread_local char g_err[512] = "";
int ctts_fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}
#define fail ctts_fail
#define CK(expr)                                                                                   \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

extern "C" const char* ctts_last_error(void) { return g_err; }
extern "C" int ctts_version(void) { return 1; }

static const int HID = 768, INTER = 3072, NHEAD = 12, HDIM = 64, NVQ = 4, NAUDIO = 626, NTEXT_MAX = 21248;

// ------------------------------------------------------------------------------------------------
struct ctts_gpt {
  ctts_gpt_weights w;
  std::vector<const void*> wqkv, wo, wgu, wd;
  std::vector<const void*> wqkv_pk, wo_pk, wgu_pk, wd_pk;   // fragment-packed copies for the decode step, or empty
  std::vector<const void*> wo_hd;                           // o_proj per attention head (perf mode), or empty
  std::vector<const void*> wqkv_x3, wo_x3, wgu_x3, wd_x3;   // parity mode: hi | lo bf16 planes in fragment order (decode32x.hip), or empty
  bool dec_x3 = false;         // parity mode: the split-bf16 planes are loaded (decode32x.hip); ctts_gen_state.proj_exact picks decode32.hip per call
  bool qkv_att = false;        // perf mode decode, <= 64 rows: QKV + attention as ONE launch (gpt.hip qkv_attention_k); env CTTS_QKV_ATT=1, OFF by default
  bool att_oproj = false;      // perf mode decode: o_proj + residual folded into the attention launch -- OPT-IN, env CTTS_ATT_OPROJ=1 (default: separate launches)
  bool dec_packed = false;     // perf mode (bf16 weights): decode.hip
  bool dec_packed32 = false;   // parity mode (f32 weights): decode32.hip
  bool heads_packed = false;   // heads GEMM on packed f32 operands (decode32.hip), both modes
  int pf_mask = 0;             // env CTTS_PF: cross-kernel weight prefetch, bit mask (1 QKV->o_proj, 16 QKV->gate/up, 2 attention->gate/up)
  int temporal_layers = 0;     // env CTTS_W_TEMPORAL_LAYERS: decode weights of layers [0, N) loaded WITHOUT the non-temporal hint (A/B)
  bool pre32_packed = true;    // parity mode: prompt pass on the packed f32 kernels (env CTTS_PRE32_PACKED=0: row-major gemm_skinny_k)
  bool embed_fold = false;     // multi-step graphs: steps 2..n take their input rows from the previous step's sampling launch (env CTTS_EMBED_FOLD=1)
  bool pre_compact = true;     // "f32x3" mode: the prompt pass over the valid prompt tokens only (env CTTS_PRE_COMPACT=0: all B * T rows)
  bool pre_x3 = true;          // "f32x3" mode: prompt pass on the LDS-tiled split-bf16 GEMM (prefill32x.hip); env CTTS_PRE_X3=0: the f32 MFMA kernels
  bool fnorm_fuse = true;      // decode: final norm + hidden capture + heads in one launch (env CTTS_FNORM_FUSE=0: separate launches)
  std::vector<const float*> ln1, ln2;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  // optional second executable graph of `multi_steps` consecutive decode steps (env CTTS_GRAPH_STEPS > 1): one hipGraphLaunch per
  // multi_steps steps instead of one per step
  hipGraph_t graph_multi = nullptr;
  hipGraphExec_t exec_multi = nullptr;
  // round 5: the same step captured for a BOUND on the live rows (ctts_gpt_graph_build_rows): every grid of the step is sized for `rows`
  // compact rows instead of B -- the attention launch loses its dead workgroups (12 per finished utterance), the 16-row projections their
  // dead row tiles.  Nothing else changes: the kernels still read the live count, so a bound that is merely >= it gives the same bits.
  struct RowsGraph { hipGraph_t graph = nullptr, gm = nullptr; hipGraphExec_t exec = nullptr, exec_multi = nullptr; };
  std::map<int, RowsGraph> rows_graphs;
  int multi_steps = 1;
  // profiling (eager decode only)
  int prof_tag = -1;
  int prof_max = 0;
  bool skip_finished = true;  // env CTTS_SKIP_FINISHED=0 restores the reference's "finished rows keep stepping"
  int n_cu = 0;               // compute units of the device when attention remainder splitting is on (env CTTS_ATT_SPLIT=1); 0 = off
  int prof_stride = 1;   // time every prof_stride-th launch of the tag
  int prof_seen = 0;
  std::vector<hipEvent_t> ev0, ev1;
  int prof_n = 0;
};

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
#define ATT_CUS_MAX 512   // upper bound of compute units the attention split state is sized for
#define QA_LAYERS_MAX 32  // layers the arrival words of the fused QKV + attention launches are sized for
#define QA_STRIDE HO_STRIDE   // kernels.hpp: ints between two arrival words
struct GptWs {
  float *x, *qkv, *ao, *act, *hfin, *logits, *ssq;
  uint16_t* xb;  // bf16 copy of the residual stream (perf mode); ao / act are reused as bf16 buffers there
  // decode step on fragment-packed operands (decode.hip): row tiles of 16 utterances
  uint16_t *xp, *aop, *actp;
  float *xp32, *aop32, *actp32;   // the same in float32 (parity mode, decode32.hip)
  float* hfinp;                   // final-norm rows in the packed f32 order (A operand of the packed heads GEMM, both modes)
  float* rstd;                    // parity mode prefill: 1 / rms of every prompt row (prefill32.hip)
  RowDesc* desc;
  float* att_part;    // attention remainder splitting: partials of the split units' pieces, and their arrival counters
  int32_t* att_cnt;
  int32_t* row_map;   // device-side compaction: this step's compact row -> utterance map (written by the step's first kernel)
  float* rope_cs;     // [Bp][64] cos[32] | sin[32] of every decode row's position, written by the step's first kernel (fused QKV + attention)
  int32_t* qa_flag;   // fused QKV + attention launches: arrival words [QA_LAYERS_MAX][12 heads], QA_STRIDE ints apart, zeroed by the step's first kernel
  float* op_part;     // attention + o_proj in one launch: [Bp][12][768] partials of the (utterance, head) units ...
  int32_t* op_cnt;    // ... and the rows' arrival counters, RIGHT BEHIND att_cnt: one memset zeroes both (cnt_bytes)
  size_t op_part_bytes;
  size_t bytes;
};
static size_t cnt_bytes(int B) { return ((size_t)ATT_CUS_MAX + ((size_t)B + 15) / 16 * 16) * sizeof(int32_t); }
static GptWs carve(void* base, int B, int T) {
  const size_t M = (size_t)B * (T > 1 ? T : 1);
  GptWs w;
  size_t off = 0;
  char* p = (char*)base;
  w.x = (float*)(p + off); off += align_up(M * HID * 4);
  w.qkv = (float*)(p + off); off += align_up(M * 3 * HID * 4);
  w.ao = (float*)(p + off); off += align_up(M * HID * 4);
  w.act = (float*)(p + off); off += align_up(M * INTER * 4);
  w.hfin = (float*)(p + off); off += align_up((size_t)B * HID * 4);
  w.logits = (float*)(p + off); off += align_up((size_t)B * NTEXT_MAX * 4);  // >= B*4*626; refine-text mode needs B*n_text
  w.ssq = (float*)(p + off); off += align_up(M * SSQ_PARTS * 4);
  w.xb = (uint16_t*)(p + off); off += align_up(M * HID * 2);
  const size_t Bp = ((size_t)B + 15) / 16 * 16;
  w.xp = (uint16_t*)(p + off); off += align_up(Bp * HID * 2);
  w.aop = (uint16_t*)(p + off); off += align_up(Bp * HID * 2);
  w.actp = (uint16_t*)(p + off); off += align_up(Bp * INTER * 2);
  // the packed f32 buffers and the row descriptors also serve the parity mode's PREFILL (M = B * T rows in 16-row tiles)
  const size_t Mp = (M + 15) / 16 * 16;
  w.xp32 = (float*)(p + off); off += align_up(Mp * HID * 4);
  w.aop32 = (float*)(p + off); off += align_up(Mp * HID * 4);
  w.actp32 = (float*)(p + off); off += align_up(Mp * INTER * 4);
  w.hfinp = (float*)(p + off); off += align_up(Bp * HID * 4);
  w.desc = (RowDesc*)(p + off); off += align_up(Mp * sizeof(RowDesc));
  w.rstd = (float*)(p + off); off += align_up(Mp * sizeof(float));
  w.row_map = (int32_t*)(p + off); off += align_up(Bp * sizeof(int32_t));
  w.att_part = (float*)(p + off); off += align_up((size_t)ATT_CUS_MAX * ATT_SPLIT_MAX * 66 * sizeof(float));
  w.att_cnt = (int32_t*)(p + off); off += align_up(cnt_bytes(B));
  w.op_cnt = w.att_cnt + ATT_CUS_MAX;
  w.op_part_bytes = Bp * NHEAD * HID * sizeof(float);
  w.op_part = (float*)(p + off); off += align_up(w.op_part_bytes);
  w.rope_cs = (float*)(p + off); off += align_up(Bp * 64 * sizeof(float));
  w.qa_flag = (int32_t*)(p + off); off += align_up((size_t)QA_LAYERS_MAX * NHEAD * QA_STRIDE * sizeof(int32_t));
  w.bytes = off;
  return w;
}

extern "C" size_t ctts_gpt_workspace_bytes(int32_t B, int32_t T) { return carve(nullptr, B, T).bytes; }

extern "C" int ctts_gpt_create(ctts_gpt** out, const ctts_gpt_weights* w) {
  if (!out || !w || w->n_layers <= 0) return fail("ctts_gpt_create: bad arguments");
  ctts_gpt* g = new ctts_gpt();
  g->w = *w;
  const int L = w->n_layers;
  g->wqkv.assign(w->wqkv, w->wqkv + L);
  g->wo.assign(w->wo, w->wo + L);
  g->wgu.assign(w->wgu, w->wgu + L);
  g->wd.assign(w->wd, w->wd + L);
  g->ln1.assign(w->ln1, w->ln1 + L);
  g->ln2.assign(w->ln2, w->ln2 + L);
  if (w->wqkv_pk && w->wo_pk && w->wgu_pk && w->wd_pk) {   // packed in the order of the weight dtype's decode kernel
    g->wqkv_pk.assign(w->wqkv_pk, w->wqkv_pk + L);
    g->wo_pk.assign(w->wo_pk, w->wo_pk + L);
    g->wgu_pk.assign(w->wgu_pk, w->wgu_pk + L);
    g->wd_pk.assign(w->wd_pk, w->wd_pk + L);
    const char* e = getenv("CTTS_DEC_PACKED");   // =0: decode on the row-major kernels (A/B)
    const bool on = !(e && atoi(e) == 0);
    g->dec_packed = on && w->weight_dtype == CTTS_BF16;
    g->dec_packed32 = on && w->weight_dtype != CTTS_BF16 && w->kv_dtype != CTTS_BF16;
  }
  { const char* e = getenv("CTTS_DEC_PACKED"); g->heads_packed = w->heads_pk != nullptr && !(e && atoi(e) == 0); }
  if (w->wqkv_x3 && w->wo_x3 && w->wgu_x3 && w->wd_x3 && w->weight_dtype != CTTS_BF16 && w->kv_dtype != CTTS_BF16) {   // (w*_pk: optional beside them)
    g->wqkv_x3.assign(w->wqkv_x3, w->wqkv_x3 + L);
    g->wo_x3.assign(w->wo_x3, w->wo_x3 + L);
    g->wgu_x3.assign(w->wgu_x3, w->wgu_x3 + L);
    g->wd_x3.assign(w->wd_x3, w->wd_x3 + L);
    g->dec_x3 = true;   // the host's choice (no planes = exact f32 MFMA); per call: ctts_gen_state.proj_exact
  }
  if (w->wo_hd && g->dec_packed) {
    g->wo_hd.assign(w->wo_hd, w->wo_hd + L);
    // OFF by default: measured on the C3 bench the fused launch costs what the two launches cost (13.9 us vs 9.07 + 4.87) and the step
    // gets 26 us SLOWER (profiles/r4b_ab_oproj.log): the 12 -> 1 hand-off through memory is a chain of dependent round trips
    const char* e = getenv("CTTS_ATT_OPROJ");
    g->att_oproj = e && atoi(e) == 1;
  }
  { const char* e = getenv("CTTS_SKIP_FINISHED"); if (e && atoi(e) == 0) g->skip_finished = false; }
  { const char* e = getenv("CTTS_FNORM_FUSE"); if (e && atoi(e) == 0) g->fnorm_fuse = false; }
  { const char* e = getenv("CTTS_W_TEMPORAL_LAYERS"); if (e) g->temporal_layers = atoi(e); }
  { const char* e = getenv("CTTS_PF"); if (e) g->pf_mask = atoi(e); }
  // OFF by default: measured on the C3 bench the fused launch is worth +0.1 ... +0.8 % (13.9 us against 5.3 + 9.1 us; more prefetch ahead of
  // the wait LOSES 4 %, none loses 4 %: profiles/r4f_ab_qkv_att_pre.log, r4g_ab_qkv_att_variants.log) -- not enough to make a launch that
  // spins on device memory the default
  { const char* e = getenv("CTTS_QKV_ATT"); g->qkv_att = e && atoi(e) == 1; }
  { const char* e = getenv("CTTS_PRE32_PACKED"); if (e && atoi(e) == 0) g->pre32_packed = false; }
  { const char* e = getenv("CTTS_PRE_X3"); if (e && atoi(e) == 0) g->pre_x3 = false; }
  { const char* e = getenv("CTTS_PRE_COMPACT"); if (e && atoi(e) == 0) g->pre_compact = false; }
  { const char* e = getenv("CTTS_EMBED_FOLD"); if (e) g->embed_fold = atoi(e) != 0; }
  {
    int dev = 0, cus = 0;
    // OFF by default: measured on the C3 bench it does not pay (attention 9.3 -> 9.8 us per launch, 1296 -> 1280 audio-s/s,
    // profiles/r2e_ab_split.log) and it makes a row's bf16 result depend on how many rows share the step
    const char* e = getenv("CTTS_ATT_SPLIT");
    if (e && atoi(e) == 1 && hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0 && cus <= ATT_CUS_MAX)
      g->n_cu = cus;
  }
  *out = g;
  return 0;
}

extern "C" void ctts_gpt_graph_destroy(ctts_gpt* g) {
  if (!g) return;
  if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
  if (g->graph) { (void)hipGraphDestroy(g->graph); g->graph = nullptr; }
  if (g->exec_multi) { (void)hipGraphExecDestroy(g->exec_multi); g->exec_multi = nullptr; }
  if (g->graph_multi) { (void)hipGraphDestroy(g->graph_multi); g->graph_multi = nullptr; }
  for (auto& kv : g->rows_graphs) {
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
    if (kv.second.exec_multi) (void)hipGraphExecDestroy(kv.second.exec_multi);
    if (kv.second.gm) (void)hipGraphDestroy(kv.second.gm);
  }
  g->rows_graphs.clear();
}

extern "C" void ctts_gpt_destroy(ctts_gpt* g) {
  if (!g) return;
  ctts_gpt_graph_destroy(g);
  for (auto e : g->ev0) (void)hipEventDestroy(e);
  for (auto e : g->ev1) (void)hipEventDestroy(e);
  delete g;
}

thread_local hipEvent_t ctts_prof_start = nullptr, ctts_prof_stop = nullptr;

// arms the start/stop events for the single kernel launch that follows (see CTTS_LAUNCH in kernels.hpp)
struct Prof {
  ctts_gpt* g; bool on;
  Prof(ctts_gpt* g_, int tag, hipStream_t, bool allow) : g(g_), on(false) {
    if (allow && g->prof_tag == tag && g->prof_n < g->prof_max && (g->prof_seen++ % g->prof_stride) == 0) {
      on = true;
      ctts_prof_start = g->ev0[g->prof_n];
      ctts_prof_stop = g->ev1[g->prof_n];
    }
  }
  ~Prof() {
    if (on) { g->prof_n++; ctts_prof_start = nullptr; ctts_prof_stop = nullptr; }
  }
};

static_assert(sizeof(SamplingRow) == sizeof(ctts_sampling_row) && sizeof(ctts_sampling_row) == 128, "ctts_sampling_row layout");
static_assert(offsetof(SamplingRow, pow_table) == offsetof(ctts_sampling_row, pow_table) &&
              offsetof(SamplingRow, min_new) == offsetof(ctts_sampling_row, min_new) &&
              offsetof(SamplingRow, rng_seed) == offsetof(ctts_sampling_row, rng_seed) &&
              offsetof(SamplingRow, rng_per_step) == offsetof(ctts_sampling_row, rng_per_step), "ctts_sampling_row layout");

static SampleArgs make_sample_args(const ctts_gen_state* s, const float* logits) {
  SampleArgs a;
  a.logits = logits; a.ids_buf = s->ids_buf; a.tcap = s->cap ? s->cap : s->T + s->max_new; a.T = s->T; a.len = s->len; a.finish = s->finish;
  a.end_idx = s->end_idx; a.q = s->q; a.nq = s->nq; a.temperature = s->temperature; a.pow_table = s->pow_table;
  a.top_p_thr = s->top_p_thr; a.use_top_p = s->use_top_p; a.top_k = s->top_k; a.use_top_k = s->use_top_k;
  a.min_new = s->min_new; a.eos = s->eos; a.row_offset = s->row_offset; a.max_input_ids = NAUDIO - 1; a.stop_at = s->stop_at;
  a.B = s->B; a.row_map = nullptr; a.n_active = nullptr; a.prompt_len = s->prompt_len; a.q_rows = s->q_batch ? s->q_batch : s->B;
  a.teacher = s->teacher_ids; a.teacher_stride = s->hid_cap ? s->hid_cap : s->max_new; a.sampled = s->sampled_ids;
  a.dbg = nullptr;
  { const char* e = getenv("CTTS_SAMPLE_DBG_PTR"); if (e) a.dbg = (long long*)strtoull(e, nullptr, 0); }   // probes only
  a.desc = nullptr; a.rng_device = s->rng_device; a.rng_per_step = s->rng_per_step; a.rng_seed = reinterpret_cast<const unsigned long long*>(s->rng_seed);
  a.rng_nonce = s->rng_nonce;
  a.margin = s->margin; a.row_base = s->row_base;
  a.rows = reinterpret_cast<const SamplingRow*>(s->row_sampling);
  memset(&a.next, 0, sizeof(a.next));
  return a;
}

// ws_T: prompt slots the workspace must hold for THIS call (a prompt chunk needs ctts_gpt_workspace_bytes(B, tc) only; the decode
// step carves for one row per utterance but keeps the prefill's carve layout, so it is checked against the geometry the caller
// allocated for: s->T unless `decode_ws_T` says otherwise)
static int check_state(const ctts_gpt* g, const ctts_gen_state* s, int ws_T = 0) {
  if (!g || !s) return fail("null engine/state");
  if (s->B <= 0 || s->T <= 0 || s->max_new <= 0) return fail("bad B/T/max_new");
  const int cap_ = s->cap ? s->cap : s->T + s->max_new;
  if (cap_ > g->w.max_pos) return fail("slot capacity T + max_new (%d) exceeds the RoPE table (%d)", cap_, g->w.max_pos);
  if (s->cap && s->T + 1 > s->cap) return fail("prompt does not fit the slot capacity");
  if (s->workspace_bytes < ctts_gpt_workspace_bytes(s->B, ws_T > 0 ? ws_T : s->T)) return fail("workspace too small");
  if (!s->rng_device && (s->nq <= 0 || !s->q)) return fail("q draws missing");
  if (s->rng_device && !s->rng_seed && !s->row_sampling) return fail("rng_device needs the rng_seed device scalar (or row_sampling)");
  if (g->w.weight_dtype == CTTS_BF16 && g->w.kv_dtype != CTTS_BF16) return fail("perf mode needs a bf16 KV cache");
  if (s->infer_text) {
    if (!g->w.emb_text || !g->w.head_text || g->w.n_text <= 0 || g->w.n_text > NTEXT_MAX) return fail("text head/embedding not loaded");
    if (s->pow_table) return fail("refine-text mode does not support a repetition penalty (the reference's own processor mis-broadcasts there)");
    if (s->eos < 0 || s->eos >= g->w.n_text) return fail("bad eos for text mode");
  }
  return 0;
}

// Device-side compaction of the decode batch: the caller passes a writable `n_active` scalar and NO row_map; the first kernel
// of every step then ranks the utterances whose finish flag is 0 (ascending slot), writes the map and the live count, and the
// step computes exactly those rows.  (With a host row_map -- slot pools -- the host stays in charge of both.)
static bool dev_compact(const ctts_gpt* g, const ctts_gen_state* s) {
  return s->row_map == nullptr && s->n_active != nullptr && g->skip_finished;
}

// the 20-layer body + heads + sampling over M = B * q_per_b rows
static bool prefill_compacts(const ctts_gpt* g, const ctts_gen_state* s) {   // the prompt pass of this call runs over the valid tokens only
  return g->w.weight_dtype != CTTS_BF16 && g->dec_x3 && !s->proj_exact && g->pre_x3 && g->pre_compact && s->row_map == nullptr &&
         s->prefill_valid_rows > 0 && s->prefill_valid_rows < s->B * s->T;
}

static int run_step(ctts_gpt* g, const ctts_gen_state* s, int q_per_b, hipStream_t st, bool prof_ok, int slot0 = 0, bool heads = true,
                    int ws_T = 0, int rows = 0, int pre_rows = 0, const EmbedNext* next = nullptr) {
  const GptWs ws = carve(s->workspace, s->B, ws_T ? ws_T : s->T);
  // `rows` (decode only): a bound on the live compact rows this step can have -- grids and M are sized for it instead of B (buffer
  // geometry, the KV cache's batch stride above all, stays B's)
  // pre_rows (whole-prompt pass, "f32x3"): the compact rows of the valid prompt tokens (prefill_compact_k wrote ws.x, ws.desc, ws.row_map = last_row)
  const int B = s->B, Bh = (q_per_b == 1 && rows > 0 && rows < s->B) ? rows : s->B, M = q_per_b == 1 ? Bh : (pre_rows > 0 ? pre_rows : B * q_per_b);
  const int cmax = s->cap ? s->cap : s->T + s->max_new;
  const int wt = g->w.weight_dtype, kt = g->w.kv_dtype;
  const size_t kv_layer = (size_t)(s->kv_batch ? s->kv_batch : B) * NHEAD * cmax * HDIM * (kt == CTTS_BF16 ? 2 : 4);
  const bool dec = q_per_b == 1;
  // decode: compact row -> slot (see GptRowMap) -- the host's map, or the one the step's first kernel derives from the finish
  // flags (device-side compaction); prefill: row group -> slot of a pool (or null)
  const int32_t* rmap = (dec && dev_compact(g, s)) ? ws.row_map : s->row_map;
  // CTTS_SKIP_FINISHED=0 with a caller that left the compaction to the device (row_map == NULL): nobody writes *n_active then,
  // so it must not be read -- every row steps, like the reference (gpt.py:512-518,592)
  const bool no_compact = dec && !g->skip_finished && s->row_map == nullptr;
  const int32_t* nact = (dec && !no_compact) ? s->n_active : nullptr;
  GptRowMap rm{q_per_b, s->len, s->kv_start, rmap, nact, (dec && g->skip_finished) ? s->finish : nullptr, nullptr, nullptr, nullptr, 0, slot0, 0};
  const bool fast = wt == CTTS_BF16;  // perf mode: bf16 activations, RMSNorm gain folded into wqkv / wgu by the loader
  const bool packed = fast && dec && g->dec_packed;   // decode step on fragment-packed operands (decode.hip)
  if (dec || pre_rows > 0) rm.desc = ws.desc;          // written by the embedding kernel at the head of the step / by prefill_compact_k
  if (dec && dev_compact(g, s)) rm.desc_covers_all = 1; // ... for every row of the grid (absent rows: b = -1)
  if (packed && g->n_cu > 0) { rm.sp_part = ws.att_part; rm.sp_cnt = ws.att_cnt; rm.sp_cus = g->n_cu; }
  if (packed) { const char* e = getenv("CTTS_ATT_DBG_PTR"); if (e) rm.dbg = (long long*)strtoull(e, nullptr, 0); }   // probes only
  // decode on packed operands: final RMSNorm + hidden capture + heads are ONE launch (decode32.hip gemm_dec32_fnorm16_k; the residual
  // stream reaches it in the packed f32 order: parity mode keeps it that way anyway, perf mode has the last down_proj write it)
  // (the fused launch reads the last down_proj's packed f32 rows: written by the x3 step and by the packed f32 step, not by the row-major one)
  const bool packed32_ = !fast && dec && ((g->dec_x3 && !s->proj_exact) || g->dec_packed32);
  const bool fuse_fnorm = dec && heads && g->fnorm_fuse && g->heads_packed && (packed || packed32_) &&
                          (s->infer_text ? g->w.head_text_pk : g->w.heads_pk) != nullptr;
  for (int l = 0; packed && l < g->w.n_layers; ++l) {
    void* kc = (char*)s->kcache + kv_layer * l;
    void* vc = (char*)s->vcache + kv_layer * l;
    DecGemmArgs d;
    memset(&d, 0, sizeof(d));
    d.M = M; d.eps = g->w.rms_eps; d.n_active = nact;
    d.force_nt = l < g->temporal_layers ? 1 : 0;   // A/B knob: the first N layers' weights with plain loads (candidates for the Infinity Cache)
#ifdef CTTS_PF_BUILD
    // cross-kernel weight prefetch (common.hpp): QKV -> this layer's o_proj; attention -> gate/up; gate/up -> down and the next layer's
    // QKV (last layer: the heads).  CTTS_PF is a bit mask (default 0 = off: every combination measured a net loss,
    // profiles/r3s_ab_prefetch.log): 1 QKV -> o_proj, 16 QKV -> gate/up, 2 attention -> gate/up
    const PfDesc pf_none{nullptr, 0, 0};
    const PfDesc pf_o{(const char*)g->wo_pk[l], 16u * HID * 2u, HID / 16u};
    const PfDesc pf_gu{(const char*)g->wgu_pk[l], 16u * HID * 2u, 2u * INTER / 16u};
    const PfDesc pf_d{(const char*)g->wd_pk[l], 16u * INTER * 2u, HID / 16u};
    const PfDesc pf_next = l + 1 < g->w.n_layers ? PfDesc{(const char*)g->wqkv_pk[l + 1], 16u * HID * 2u, 3u * HID / 16u}
                           : (fuse_fnorm && !s->infer_text) ? PfDesc{(const char*)g->w.heads_pk, 16u * HID * 4u, (NVQ * NAUDIO + 15u) / 16u} : pf_none;
    d.pf[0] = (g->pf_mask & 1) ? pf_o : pf_none; d.pf[1] = (g->pf_mask & 16) ? pf_gu : pf_none;
    rm.pf = (g->pf_mask & 2) ? pf_gu : pf_none;
#endif
    // RMSNorm scale + QKV + RoPE + KV append
    d.Ap = ws.xp; d.Wp = (const uint16_t*)g->wqkv_pk[l]; d.N = 3 * HID; d.K = HID; d.ssq_in = ws.ssq; d.epi = FEPI_QKV_ROPE;
    d.C32 = ws.qkv; d.ldc = 3 * HID; d.desc = ws.desc; d.cos_t = g->w.rope_cos; d.sin_t = g->w.rope_sin;
    d.kc = (uint16_t*)kc; d.vc = (uint16_t*)vc; d.cmax = cmax;
    const bool fuse_qa = g->qkv_att && M <= 64 && kv_layer < ((size_t)1 << 31) && g->w.n_layers <= QA_LAYERS_MAX && g->n_cu == 0 && g->pf_mask == 0 && !(g->att_oproj) && rm.dbg == nullptr;
    bool need_o = true;   // o_proj + residual as its own launch
    if (fuse_qa) {   // QKV + attention: one launch (gpt.hip qkv_attention_k)
      d.ho_flag = ws.qa_flag + (size_t)l * NHEAD * QA_STRIDE; rm.qf_flag = d.ho_flag; d.rope_cs = ws.rope_cs; rm.qf_kv_bytes = (int)kv_layer;
      Prof p(g, 3, st, prof_ok);
      CK(launch_qkv_attention(d, kc, vc, cmax, ws.aop, rm, M, st));
    } else {
      { Prof p(g, 1, st, prof_ok); CK(launch_gemm_dec(d, st)); }
      if (g->att_oproj && g->n_cu == 0) {   // attention + o_proj + residual: one launch (gpt.hip attention_k<OPJ>)
        rm.wo_h = (const uint16_t*)g->wo_hd[l]; rm.op_part = ws.op_part; rm.op_part_bytes = (int)ws.op_part_bytes; rm.op_cnt = ws.op_cnt;
        rm.x32 = ws.x; rm.xp = ws.xp; rm.ssq = ws.ssq;
        Prof p(g, 3, st, prof_ok);
        CK(launch_attention_oproj(ws.qkv, kc, vc, cmax, rm, M, st));
        need_o = false;
      } else {
        Prof p(g, 3, st, prof_ok);
        CK(launch_attention(ws.qkv, kc, vc, kt, cmax, ws.aop, 2, rm, M, st));
      }
    }
    if (need_o) {
      d.Ap = ws.aop; d.Wp = (const uint16_t*)g->wo_pk[l]; d.N = HID; d.ssq_in = nullptr; d.epi = FEPI_RES; d.C32 = ws.x; d.ldc = HID;
      d.Cp = ws.xp; d.kch_out = HID / 32; d.ssq_out = ws.ssq; d.ho_flag = nullptr;
      Prof p(g, 4, st, prof_ok);
      CK(launch_gemm_dec(d, st));
    }
    d.Ap = ws.xp; d.Wp = (const uint16_t*)g->wgu_pk[l]; d.N = INTER; d.ssq_in = ws.ssq; d.epi = FEPI_SILU; d.C32 = nullptr;
    d.Cp = ws.actp; d.kch_out = INTER / 32; d.ssq_out = nullptr;
#ifdef CTTS_PF_BUILD
    d.pf[0] = pf_none; d.pf[1] = pf_none; (void)pf_d; (void)pf_next;   // (gate/up has no auxiliary wave: see decode.hip)
#endif
    { Prof p(g, 5, st, prof_ok); CK(launch_gemm_dec(d, st)); }
    d.Ap = ws.actp; d.Wp = (const uint16_t*)g->wd_pk[l]; d.N = HID; d.K = INTER; d.ssq_in = nullptr; d.epi = FEPI_RES; d.C32 = ws.x;
    d.ldc = HID; d.Cp = ws.xp; d.kch_out = HID / 32; d.ssq_out = ws.ssq;
    d.Cp32 = (fuse_fnorm && l == g->w.n_layers - 1) ? ws.xp32 : nullptr;   // operand of the fused final-norm + heads launch
    { Prof p(g, 6, st, prof_ok); CK(launch_gemm_dec(d, st)); }
  }
  for (int l = 0; fast && !packed && l < g->w.n_layers; ++l) {
    void* kc = (char*)s->kcache + kv_layer * l;
    void* vc = (char*)s->vcache + kv_layer * l;
    uint16_t* aob = (uint16_t*)ws.ao;
    uint16_t* actb = (uint16_t*)ws.act;
    FastGemmArgs f;
    memset(&f, 0, sizeof(f));
    f.M = M; f.eps = g->w.rms_eps; f.n_active = nact; f.row_map = rmap; f.slot0 = slot0;
    // RMSNorm + QKV + RoPE + KV append in one launch (q/k weight rows are permuted by the loader)
    f.A = ws.xb; f.lda = HID; f.W = (const uint16_t*)g->wqkv[l]; f.N = 3 * HID; f.K = HID; f.ssq_in = ws.ssq; f.epi = FEPI_QKV_ROPE;
    f.C32 = ws.qkv; f.ldc = 3 * HID;
    f.q_per_b = q_per_b; f.len = s->len; f.kv_start = s->kv_start; f.cos_t = g->w.rope_cos; f.sin_t = g->w.rope_sin;
    f.kc = (uint16_t*)kc; f.vc = (uint16_t*)vc; f.cmax = cmax;
    { Prof p(g, 1, st, prof_ok); CK(launch_gemm_fast(f, st)); }
    { Prof p(g, 3, st, prof_ok); CK(launch_attention(ws.qkv, kc, vc, kt, cmax, aob, 1, rm, M, st)); }
    f.A = aob; f.W = (const uint16_t*)g->wo[l]; f.N = HID; f.K = HID; f.ssq_in = nullptr; f.epi = FEPI_RES; f.C32 = ws.x; f.ldc = HID;
    f.Cb = ws.xb; f.ldcb = HID; f.ssq_out = ws.ssq;
    { Prof p(g, 4, st, prof_ok); CK(launch_gemm_fast(f, st)); }
    f.A = ws.xb; f.W = (const uint16_t*)g->wgu[l]; f.N = INTER; f.K = HID; f.ssq_in = ws.ssq; f.epi = FEPI_SILU; f.C32 = nullptr;
    f.Cb = actb; f.ldcb = INTER; f.ssq_out = nullptr;
    { Prof p(g, 5, st, prof_ok); CK(launch_gemm_fast(f, st)); }
    f.A = actb; f.lda = INTER; f.W = (const uint16_t*)g->wd[l]; f.N = HID; f.K = INTER; f.ssq_in = nullptr; f.epi = FEPI_RES;
    f.C32 = ws.x; f.ldc = HID; f.Cb = ws.xb; f.ldcb = HID; f.ssq_out = ws.ssq;
    { Prof p(g, 6, st, prof_ok); CK(launch_gemm_fast(f, st)); }
  }
  // parity mode decode step on SPLIT-bf16 operands (decode32x.hip): hi | lo planes in the buffers the f32 kernels use for their packed
  // operands (same bytes: 2 planes x 2 B), the heads' packed f32 operand in ws.hfinp
  const bool x3 = !fast && dec && g->dec_x3 && !s->proj_exact;
  const size_t Bp16 = ((size_t)M + 15) / 16 * 16;
  for (int l = 0; x3 && l < g->w.n_layers; ++l) {
    void* kc = (char*)s->kcache + kv_layer * l;
    void* vc = (char*)s->vcache + kv_layer * l;
    uint16_t* xpx = reinterpret_cast<uint16_t*>(ws.xp32);
    uint16_t* aopx = reinterpret_cast<uint16_t*>(ws.aop32);
    uint16_t* actx = reinterpret_cast<uint16_t*>(ws.actp32);
    Dec32xArgs d;
    memset(&d, 0, sizeof(d));
    d.M = M; d.eps = g->w.rms_eps; d.n_active = nact;
    // RMSNorm (gain folded into the weights, 1 / rms on the accumulator) + QKV + RoPE + KV append
    d.Ap = xpx; d.a_plane = Bp16 * HID; d.Wp = (const uint16_t*)g->wqkv_x3[l]; d.w_plane = (size_t)3 * HID * HID; d.N = 3 * HID; d.K = HID;
    d.rms = 1; d.X = ws.x; d.ldx = HID; d.ssq_in = ws.ssq; d.rope_cs = ws.rope_cs; d.epi = D32_EPI_QKV_ROPE; d.C = ws.qkv; d.ldc = 3 * HID; d.desc = ws.desc;
    d.cos_t = g->w.rope_cos; d.sin_t = g->w.rope_sin; d.kc = (float*)kc; d.vc = (float*)vc; d.cmax = cmax;
    { Prof p(g, 1, st, prof_ok); CK(launch_gemm_dec32x(d, st)); }
    rm.x3_plane = Bp16 * HID;
    { Prof p(g, 3, st, prof_ok); CK(launch_attention(ws.qkv, kc, vc, kt, cmax, aopx, 4, rm, M, st)); }
    // o_proj + residual
    d.Ap = aopx; d.a_plane = Bp16 * HID; d.Wp = (const uint16_t*)g->wo_x3[l]; d.w_plane = (size_t)HID * HID; d.N = HID; d.rms = 0; d.X = nullptr;
    d.ssq_in = nullptr; d.ssq_out = ws.ssq;
    d.epi = EPI_RES; d.C = ws.x; d.ldc = HID; d.res = ws.x; d.ldr = HID; d.Cp = xpx; d.c_plane = Bp16 * HID; d.kch_out = HID / 32;
    { Prof p(g, 4, st, prof_ok); CK(launch_gemm_dec32x(d, st)); }
    // RMSNorm + gate/up + SiLU*up
    d.Ap = xpx; d.a_plane = Bp16 * HID; d.Wp = (const uint16_t*)g->wgu_x3[l]; d.w_plane = (size_t)2 * INTER * HID; d.N = INTER; d.rms = 1; d.X = ws.x;
    d.ssq_in = ws.ssq; d.ssq_out = nullptr;
    d.epi = EPI_SILU_MUL; d.C = nullptr; d.res = nullptr; d.Cp = actx; d.c_plane = Bp16 * INTER; d.kch_out = INTER / 32;
    { Prof p(g, 5, st, prof_ok); CK(launch_gemm_dec32x(d, st)); }
    // down_proj + residual (last layer: also the packed f32 rows the fused final-norm + heads launch reads)
    d.Ap = actx; d.a_plane = Bp16 * INTER; d.Wp = (const uint16_t*)g->wd_x3[l]; d.w_plane = (size_t)HID * INTER; d.N = HID; d.K = INTER; d.rms = 0;
    d.ssq_in = nullptr; d.ssq_out = ws.ssq;
    d.X = nullptr; d.epi = EPI_RES; d.C = ws.x; d.ldc = HID; d.res = ws.x; d.ldr = HID; d.Cp = xpx; d.c_plane = Bp16 * HID; d.kch_out = HID / 32;
    d.Cp32 = (fuse_fnorm && l == g->w.n_layers - 1) ? ws.hfinp : nullptr; d.kch32_out = HID / 16;
    { Prof p(g, 6, st, prof_ok); CK(launch_gemm_dec32x(d, st)); }
  }
  const bool packed32 = !fast && dec && g->dec_packed32 && !x3;   // parity mode decode step on fragment-packed f32 operands (decode32.hip)
  for (int l = 0; packed32 && l < g->w.n_layers; ++l) {
    void* kc = (char*)s->kcache + kv_layer * l;
    void* vc = (char*)s->vcache + kv_layer * l;
    Dec32Args d;
    memset(&d, 0, sizeof(d));
    d.M = M; d.eps = g->w.rms_eps; d.n_active = nact;
    // RMSNorm + QKV
    d.Ap = ws.xp32; d.Wp = (const float*)g->wqkv_pk[l]; d.N = 3 * HID; d.K = HID; d.X = ws.x; d.ldx = HID; d.norm_w = g->ln1[l];
    // ... + RoPE + KV append in the epilogue (q / k weight rows of the packed copy are permuted by the loader)
    d.epi = D32_EPI_QKV_ROPE; d.C = ws.qkv; d.ldc = 3 * HID; d.desc = ws.desc; d.cos_t = g->w.rope_cos; d.sin_t = g->w.rope_sin;
    d.kc = (float*)kc; d.vc = (float*)vc; d.cmax = cmax;
    { Prof p(g, 1, st, prof_ok); CK(launch_gemm_dec32(d, st)); }
    { Prof p(g, 3, st, prof_ok); CK(launch_attention(ws.qkv, kc, vc, kt, cmax, ws.aop32, 3, rm, M, st)); }
    // o_proj + residual
    d.Ap = ws.aop32; d.Wp = (const float*)g->wo_pk[l]; d.N = HID; d.X = nullptr; d.norm_w = nullptr; d.epi = EPI_RES; d.C = ws.x; d.ldc = HID;
    d.res = ws.x; d.ldr = HID; d.Cp = ws.xp32; d.kch_out = HID / 16;
    { Prof p(g, 4, st, prof_ok); CK(launch_gemm_dec32(d, st)); }
    // RMSNorm + gate/up + SiLU*up
    d.Ap = ws.xp32; d.Wp = (const float*)g->wgu_pk[l]; d.N = INTER; d.X = ws.x; d.norm_w = g->ln2[l]; d.epi = EPI_SILU_MUL; d.C = nullptr;
    d.res = nullptr; d.Cp = ws.actp32; d.kch_out = INTER / 16;
    { Prof p(g, 5, st, prof_ok); CK(launch_gemm_dec32(d, st)); }
    // down_proj + residual
    d.Ap = ws.actp32; d.Wp = (const float*)g->wd_pk[l]; d.N = HID; d.K = INTER; d.X = nullptr; d.norm_w = nullptr; d.epi = EPI_RES;
    d.C = ws.x; d.ldc = HID; d.res = ws.x; d.ldr = HID; d.Cp = ws.xp32; d.kch_out = HID / 16;
    { Prof p(g, 6, st, prof_ok); CK(launch_gemm_dec32(d, st)); }
  }
  // parity mode PREFILL on packed operands (round 3, prefill32.hip): the prompt rows are packed once, every projection is a
  // register-blocked launch over fragment-order operands (one wave = 32 x 32 outputs x the 4 k-chunk classes; same chunk order per
  // class, same ((s0+s1)+s2)+s3, 1/rms per row from wave_row_rstd like gemm_skinny_k), RoPE + KV append run in the QKV epilogue from
  // per-row descriptors, attention writes its output packed.  Bit-identical to the row-major prefill (CTTS_PRE32_PACKED=0), which
  // the goldens were made with.  (The decode kernels' generic 64-row body was tried first: no faster than row-major at this M.)
  // "f32x3" mode (round 6): the prompt rows go through the row-major path below with its four projections on the LDS-tiled split-bf16
  // GEMM (prefill32x.hip) -- 3 bf16 MFMAs per product instead of f32 MFMA at a sixteenth of the rate; an exact call keeps the f32 kernels
  const bool pre_x3 = !fast && !dec && g->dec_x3 && !s->proj_exact && g->pre_x3;
  const bool pre32 = !fast && !dec && g->dec_packed32 && g->pre32_packed && !pre_x3;
  if (pre32) {
    CK(launch_prefill_prep32(ws.x, ws.xp32, ws.desc, q_per_b, slot0, s->kv_start, s->row_map, M, st));
  }
  for (int l = 0; pre32 && l < g->w.n_layers; ++l) {
    void* kc = (char*)s->kcache + kv_layer * l;
    void* vc = (char*)s->vcache + kv_layer * l;
    Dec32Args d;
    memset(&d, 0, sizeof(d));
    d.M = M; d.eps = g->w.rms_eps; d.n_active = nullptr;
    CK(launch_rows_rstd32(ws.x, HID, M, g->w.rms_eps, ws.rstd, st));
    d.Ap = ws.xp32; d.Wp = (const float*)g->wqkv_pk[l]; d.N = 3 * HID; d.K = HID; d.norm_w = g->ln1[l];
    d.epi = D32_EPI_QKV_ROPE; d.C = ws.qkv; d.ldc = 3 * HID; d.desc = ws.desc; d.cos_t = g->w.rope_cos; d.sin_t = g->w.rope_sin;
    d.kc = (float*)kc; d.vc = (float*)vc; d.cmax = cmax;
    CK(launch_gemm_pre32(d, ws.rstd, st));
    CK(launch_attention(ws.qkv, kc, vc, kt, cmax, ws.aop32, 3, rm, M, st));
    d.Ap = ws.aop32; d.Wp = (const float*)g->wo_pk[l]; d.N = HID; d.norm_w = nullptr; d.epi = EPI_RES; d.C = ws.x; d.ldc = HID;
    d.res = ws.x; d.ldr = HID; d.Cp = ws.xp32; d.kch_out = HID / 16;
    CK(launch_gemm_pre32(d, nullptr, st));
    CK(launch_rows_rstd32(ws.x, HID, M, g->w.rms_eps, ws.rstd, st));
    d.Ap = ws.xp32; d.Wp = (const float*)g->wgu_pk[l]; d.N = INTER; d.norm_w = g->ln2[l]; d.epi = EPI_SILU_MUL; d.C = nullptr;
    d.res = nullptr; d.Cp = ws.actp32; d.kch_out = INTER / 16;
    CK(launch_gemm_pre32(d, ws.rstd, st));
    d.Ap = ws.actp32; d.Wp = (const float*)g->wd_pk[l]; d.N = HID; d.K = INTER; d.norm_w = nullptr; d.epi = EPI_RES;
    d.C = ws.x; d.ldc = HID; d.res = ws.x; d.ldr = HID; d.Cp = ws.xp32; d.kch_out = HID / 16;
    CK(launch_gemm_pre32(d, nullptr, st));
  }
  for (int l = 0; !fast && !packed32 && !pre32 && !x3 && l < g->w.n_layers; ++l) {
    void* kc = (char*)s->kcache + kv_layer * l;
    void* vc = (char*)s->vcache + kv_layer * l;
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.taps = 1;
    a.n_active = nact;
    // RMSNorm + QKV
    a.A = ws.x; a.lda = HID; a.W = g->wqkv[l]; a.C = ws.qkv; a.ldc = 3 * HID; a.M = M; a.N = 3 * HID; a.K = HID; a.wt = wt;
    a.epi = EPI_STORE; a.norm_w = g->ln1[l]; a.eps = g->w.rms_eps;
    if (pre_x3) { CK(launch_rows_rstd32(ws.x, HID, M, g->w.rms_eps, ws.rstd, st)); CK(launch_gemm_pre_x3(a, ws.rstd, st)); }
    else { Prof p(g, 1, st, prof_ok); CK(launch_gemm_skinny(a, st)); }
    { Prof p(g, 2, st, prof_ok); CK(launch_rope_append(ws.qkv, kc, vc, kt, cmax, g->w.rope_cos, g->w.rope_sin, rm, M, st)); }
    { Prof p(g, 3, st, prof_ok); CK(launch_attention(ws.qkv, kc, vc, kt, cmax, ws.ao, 0, rm, M, st)); }
    // o_proj + residual
    a.A = ws.ao; a.lda = HID; a.W = g->wo[l]; a.C = ws.x; a.ldc = HID; a.N = HID; a.K = HID; a.epi = EPI_RES; a.norm_w = nullptr;
    a.res = ws.x; a.ldr = HID;
    if (pre_x3) CK(launch_gemm_pre_x3(a, nullptr, st));
    else { Prof p(g, 4, st, prof_ok); CK(launch_gemm_skinny(a, st)); }
    // RMSNorm + gate/up + SiLU*up
    a.A = ws.x; a.W = g->wgu[l]; a.C = ws.act; a.ldc = INTER; a.N = INTER; a.K = HID; a.epi = EPI_SILU_MUL; a.norm_w = g->ln2[l];
    a.res = nullptr;
    if (pre_x3) { CK(launch_rows_rstd32(ws.x, HID, M, g->w.rms_eps, ws.rstd, st)); CK(launch_gemm_pre_x3(a, ws.rstd, st)); }
    else { Prof p(g, 5, st, prof_ok); CK(launch_gemm_skinny(a, st)); }
    // down_proj + residual
    a.A = ws.act; a.lda = INTER; a.W = g->wd[l]; a.C = ws.x; a.ldc = HID; a.N = HID; a.K = INTER; a.epi = EPI_RES; a.norm_w = nullptr;
    a.res = ws.x; a.ldr = HID;
    if (pre_x3) CK(launch_gemm_pre_x3(a, nullptr, st));
    else { Prof p(g, 6, st, prof_ok); CK(launch_gemm_skinny(a, st)); }
  }
  if (!heads) return 0;   // a prompt chunk that is not the last one: its K/V rows are in the cache, nothing is sampled
  if (fuse_fnorm) {
    const int nlog = s->infer_text ? g->w.n_text : NVQ * NAUDIO;
    Dec32Args d;
    memset(&d, 0, sizeof(d));
    d.Ap = x3 ? ws.hfinp : ws.xp32; d.Wp = s->infer_text ? g->w.head_text_pk : g->w.heads_pk; d.M = Bh; d.N = (nlog + 15) / 16 * 16; d.K = HID; d.n_active = nact;
    d.epi = EPI_STORE; d.C = ws.logits; d.ldc = nlog; d.n_cols = nlog;
    d.fnorm = 1; d.norm_w = g->w.norm; d.eps = g->w.rms_eps; d.desc = ws.desc; d.hid = s->hiddens; d.hid_cap = s->hid_cap ? s->hid_cap : s->max_new;
    d.T = s->T; d.prompt_len = s->prompt_len;
    Prof p(g, 8, st, prof_ok);
    CK(launch_gemm_dec32(d, st));
  } else {
  { Prof p(g, 7, st, prof_ok);
    CK(launch_final_norm(ws.x, q_per_b, g->w.norm, g->w.rms_eps, ws.hfin, s->hiddens, s->hid_cap ? s->hid_cap : s->max_new, s->len, s->T, Bh, rmap,
                         nact, s->prompt_len, st, ws.hfinp, pre_rows > 0 ? ws.row_map : nullptr)); }
  {
    const int nlog = s->infer_text ? g->w.n_text : NVQ * NAUDIO;   // gpt.py:439-440 text head | :441-454 four code heads
    const float* hpk = s->infer_text ? g->w.head_text_pk : g->w.heads_pk;
    if (g->heads_packed && hpk != nullptr) {   // same arithmetic as the row-major kernel below, operands in fragment order
      Dec32Args d;
      memset(&d, 0, sizeof(d));
      d.Ap = ws.hfinp; d.Wp = hpk; d.M = Bh; d.N = (nlog + 15) / 16 * 16; d.K = HID; d.n_active = nact; d.epi = EPI_STORE;
      d.C = ws.logits; d.ldc = nlog; d.n_cols = nlog;
      Prof p(g, 8, st, prof_ok);
      CK(launch_gemm_dec32(d, st));
    } else {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.taps = 1;
    a.A = ws.hfin; a.lda = HID; a.W = s->infer_text ? g->w.head_text : g->w.heads; a.C = ws.logits; a.ldc = nlog; a.M = Bh; a.N = nlog;
    a.K = HID; a.wt = WT_F32; a.epi = EPI_STORE; a.n_active = nact;
    Prof p(g, 8, st, prof_ok);
    CK(launch_gemm_skinny(a, st));
    }
  }
  }
  {
    Prof p(g, 9, st, prof_ok);
    SampleArgs sa = make_sample_args(s, ws.logits);
    sa.B = Bh;   // (the grid; q_rows keeps the batch geometry)
    sa.row_map = rmap; sa.n_active = nact;
    if (dec && dev_compact(g, s)) sa.desc = ws.desc;   // one load instead of the n_active -> row_map -> len chain
    if (next != nullptr && sa.desc != nullptr && !s->infer_text) sa.next = *next;   // the next step's first kernel, folded into this launch
    if (s->infer_text) CK(launch_sample_text(sa, g->w.n_text, st));
    else CK(launch_sample(sa, st));
  }
  return 0;
}

extern "C" int ctts_gpt_prefill(ctts_gpt* g, const ctts_gen_state* s, const float* emb, void* stream) {
  if (check_state(g, s)) return -1;
  CttsDeviceGuard dg(stream);
  hipStream_t st = (hipStream_t)stream;
  const GptWs ws = carve(s->workspace, s->B, s->T);
  CK(hipMemsetAsync(ws.att_cnt, 0, cnt_bytes(s->B), st));   // arrival counters of the attention split
  if (prefill_compacts(g, s)) {
    // the prompt pass over the valid prompt tokens only: their embeddings gathered into consecutive rows, descriptors per row
    CK(launch_prefill_compact(emb, ws.x, ws.desc, ws.row_map, s->B, s->T, s->kv_start, st));
    if (run_step(g, s, s->T, st, false, 0, true, 0, 0, s->prefill_valid_rows)) return -1;
    CK(hipMemsetAsync(carve(s->workspace, s->B, 1).att_cnt, 0, cnt_bytes(s->B), st));
    return 0;
  }
  CK(hipMemcpyAsync(ws.x, emb, (size_t)s->B * s->T * HID * 4, hipMemcpyDeviceToDevice, st));
  if (g->w.weight_dtype == CTTS_BF16) CK(launch_rows_prep(ws.x, ws.xb, ws.ssq, s->B * s->T, st));
  if (run_step(g, s, s->T, st, false)) return -1;
  // arrival counters of the attention split at the place the DECODE steps carve them (one row per utterance), once the
  // prompt-sized buffers above are dead
  CK(hipMemsetAsync(carve(s->workspace, s->B, 1).att_cnt, 0, cnt_bytes(s->B), st));
  return 0;
}

extern "C" int ctts_gpt_prefill_chunk(ctts_gpt* g, const ctts_gen_state* s, const float* emb_chunk, int32_t t0, int32_t tc, int32_t last,
                                      void* stream) {
  if (check_state(g, s, tc > 0 ? tc : 1)) return -1;
  if (t0 < 0 || tc <= 0 || t0 + tc > s->T || (last && t0 + tc != s->T)) return fail("ctts_gpt_prefill_chunk: bad chunk [%d, %d) of a %d-slot prompt", t0, t0 + tc, s->T);
  if (s->workspace_bytes < ctts_gpt_workspace_bytes(s->B, tc)) return fail("workspace too small for the chunk");
  CttsDeviceGuard dg(stream);
  hipStream_t st = (hipStream_t)stream;
  const GptWs ws = carve(s->workspace, s->B, tc);
  CK(hipMemcpyAsync(ws.x, emb_chunk, (size_t)s->B * tc * HID * 4, hipMemcpyDeviceToDevice, st));
  if (g->w.weight_dtype == CTTS_BF16) CK(launch_rows_prep(ws.x, ws.xb, ws.ssq, s->B * tc, st));
  if (run_step(g, s, tc, st, false, t0, last != 0, tc)) return -1;
  // the decode steps carve the workspace for one row per utterance: zero THEIR attention-split arrival counters once the
  // chunk-sized buffers above are dead
  if (last) CK(hipMemsetAsync(carve(s->workspace, s->B, 1).att_cnt, 0, cnt_bytes(s->B), st));
  return 0;
}

// The decode step carves the workspace for ONE row per utterance (ctts_gpt_workspace_bytes(B, 1)) whatever the prompt length was: a
// caller that prefills in chunks of tc slots needs max(bytes(B, tc), bytes(B, 1)), not bytes(B, T).  Nothing in the workspace
// survives from the prefill into the decode steps (all generation state lives in ctts_gen_state's own arrays).
// skip_embed / fold_next (multi-step graphs, env CTTS_EMBED_FOLD=1): step i > 0 of the group finds its input rows written by step i - 1's
// sampling launch (EmbedNext), step i < n - 1 writes them for step i + 1
static int decode_body(ctts_gpt* g, const ctts_gen_state* s, hipStream_t st, bool prof_ok, int rows = 0, bool skip_embed = false,
                       bool fold_next = false) {
  const GptWs ws = carve(s->workspace, s->B, 1);
  EmbedNext nx;
  memset(&nx, 0, sizeof(nx));
  { Prof p(g, 0, st, prof_ok); const bool fast = g->w.weight_dtype == CTTS_BF16;
    const bool packed = fast && g->dec_packed;
    const bool dc = dev_compact(g, s);
    const bool x3 = !fast && g->dec_x3 && !s->proj_exact;   // split-bf16 parity mode: the residual rows as hi | lo planes (decode32x.hip)
    StepPrep sp{ws.desc, s->kv_start, g->skip_finished ? s->finish : nullptr, (packed || x3) ? 1 : 0, (!fast && g->dec_packed32 && !x3) ? ws.xp32 : nullptr,
                dc ? ws.row_map : nullptr,
                dc ? const_cast<int32_t*>(s->n_active) : nullptr, dc ? s->order : nullptr,
                ((packed && g->qkv_att && g->w.n_layers <= QA_LAYERS_MAX) || x3) ? ws.rope_cs : nullptr, g->w.rope_cos, g->w.rope_sin,
                // the arrival words are sized for QA_LAYERS_MAX layers: the same predicate as `fuse_qa` in run_step (a deeper model
                // never takes the fused launch and must not zero past the carve either)
                (packed && g->qkv_att && g->w.n_layers <= QA_LAYERS_MAX) ? ws.qa_flag : nullptr, g->w.n_layers * NHEAD, QA_STRIDE};
    const int32_t* nact0 = (!g->skip_finished && s->row_map == nullptr) ? nullptr : s->n_active;
    uint16_t* xb = fast ? (packed ? ws.xp : ws.xb) : x3 ? reinterpret_cast<uint16_t*>(ws.xp32) : nullptr;
    if (x3) sp.xb_lo_plane = ((size_t)((rows > 0 && rows < s->B) ? rows : s->B) + 15) / 16 * 16 * HID;   // = run_step's plane stride for this bound
    const bool foldable = dc && !s->infer_text && sp.zero_p == nullptr;
    if (fold_next && foldable) { nx.emb_code = g->w.emb_code; nx.x = ws.x; nx.xb = xb; nx.ssq = (fast || x3) ? ws.ssq : nullptr; nx.sp = sp; }
    if (skip_embed && foldable) { /* written by the previous step's sampling launch */ }
    else if (s->infer_text)
      CK(launch_embed_text(g->w.emb_text, g->w.n_text, s->ids_buf, s->cap ? s->cap : s->T + s->max_new, s->len, ws.x, xb,
                           (fast || x3) ? ws.ssq : nullptr, s->B, s->row_map, nact0, st, &sp));
    else
      CK(launch_embed_codes(g->w.emb_code, s->ids_buf, s->cap ? s->cap : s->T + s->max_new, s->len, ws.x, xb, (fast || x3) ? ws.ssq : nullptr, s->B,
                            s->row_map, nact0, st, &sp)); }
  return run_step(g, s, 1, st, prof_ok, 0, true, 1, rows, 0, nx.x != nullptr ? &nx : nullptr);
}

extern "C" int ctts_gpt_decode_step(ctts_gpt* g, const ctts_gen_state* s, void* stream) {
  if (check_state(g, s, 1)) return -1;
  CttsDeviceGuard dg(stream);
  return decode_body(g, s, (hipStream_t)stream, true);
}

// captures decode_body (rows bound `rows`, 0 = the whole batch) as a 1-step graph and as a graph of g->multi_steps steps
static int capture_graphs(ctts_gpt* g, const ctts_gen_state* s, hipStream_t st, int rows, hipGraph_t* graph, hipGraphExec_t* exec, hipGraph_t* gm,
                          hipGraphExec_t* exec_multi) {
  CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = decode_body(g, s, st, false, rows);
  hipGraph_t gr = nullptr;
  hipError_t e = hipStreamEndCapture(st, &gr);
  if (rc != 0) { if (gr) (void)hipGraphDestroy(gr); return -1; }
  if (e != hipSuccess) return fail("hipStreamEndCapture: %s", hipGetErrorString(e));
  *graph = gr;
  CK(hipGraphInstantiate(exec, gr, nullptr, nullptr, 0));
  if (g->multi_steps > 1) {
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc2 = 0;
    for (int i = 0; i < g->multi_steps && rc2 == 0; ++i)
      rc2 = decode_body(g, s, st, false, rows, g->embed_fold && i > 0, g->embed_fold && i + 1 < g->multi_steps);
    hipGraph_t g2 = nullptr;
    hipError_t e3 = hipStreamEndCapture(st, &g2);
    if (rc2 != 0) { if (g2) (void)hipGraphDestroy(g2); return -1; }
    if (e3 != hipSuccess) return fail("hipStreamEndCapture (multi-step graph): %s", hipGetErrorString(e3));
    *gm = g2;
    CK(hipGraphInstantiate(exec_multi, g2, nullptr, nullptr, 0));
  }
  return 0;
}

extern "C" int ctts_gpt_graph_build(ctts_gpt* g, const ctts_gen_state* s, void* stream) {
  if (check_state(g, s, 1)) return -1;
  CttsDeviceGuard dg(stream);
  ctts_gpt_graph_destroy(g);
  hipStream_t st = (hipStream_t)stream;
  if (st == nullptr) return fail("graph capture needs a non-default stream");
  {  // the decode workspace may never have seen a prefill (slot pools prefill into their own): zero the arrival counters of the
     // attention split once, stream-ordered before anything the graph will run
    const GptWs ws = carve(s->workspace, s->B, 1);
    CK(hipMemsetAsync(ws.att_cnt, 0, cnt_bytes(s->B), st));
  }
  // default 8 steps per launch of the multi-step graph: +0.5 % on the C3 bench over one hipGraphLaunch per step
  // (profiles/r3b_ab_fnorm_graphsteps.log: 1325 -> 1331-1334 audio-s/s with 8, 1328-1331 with 16)
  { const char* e2 = getenv("CTTS_GRAPH_STEPS"); g->multi_steps = e2 ? atoi(e2) : 8; }
  if (g->multi_steps < 1 || g->multi_steps > 64) g->multi_steps = 1;
  return capture_graphs(g, s, st, 0, &g->graph, &g->exec, &g->graph_multi, &g->exec_multi);
}

// The same step for a bound on the live rows (see ctts_gpt::rows_graphs).  Needs ctts_gpt_graph_build of the same state first (it owns the
// geometry; ctts_gpt_graph_build / _destroy drop every bounded graph too).  rows >= B: nothing to build (the plain graph is that graph).
extern "C" int ctts_gpt_graph_build_rows(ctts_gpt* g, const ctts_gen_state* s, int32_t rows, void* stream) {
  if (check_state(g, s, 1)) return -1;
  if (!g->exec) return fail("ctts_gpt_graph_build_rows: build the plain graph first");
  if (rows <= 0) return fail("ctts_gpt_graph_build_rows: bad bound");
  if (rows >= s->B || g->rows_graphs.count(rows)) return 0;
  CttsDeviceGuard dg(stream);
  hipStream_t st = (hipStream_t)stream;
  if (st == nullptr) return fail("graph capture needs a non-default stream");
  ctts_gpt::RowsGraph rg;
  if (capture_graphs(g, s, st, rows, &rg.graph, &rg.exec, &rg.gm, &rg.exec_multi)) return -1;
  g->rows_graphs[rows] = rg;
  return 0;
}

extern "C" int ctts_gpt_graph_launch(ctts_gpt* g, int32_t n_steps, void* stream) {
  if (!g || !g->exec) return fail("no captured graph");
  CttsDeviceGuard dg(stream);
  int left = n_steps;
  while (g->exec_multi && left >= g->multi_steps) { CK(hipGraphLaunch(g->exec_multi, (hipStream_t)stream)); left -= g->multi_steps; }
  for (int i = 0; i < left; ++i) CK(hipGraphLaunch(g->exec, (hipStream_t)stream));
  return 0;
}

// n_steps replays of the step captured for the bound `rows` (the caller guarantees live rows <= rows for all of them; rows >= B or a
// bound that was never built: the plain graph)
extern "C" int ctts_gpt_graph_launch_rows(ctts_gpt* g, int32_t n_steps, int32_t rows, void* stream) {
  if (!g || !g->exec) return fail("no captured graph");
  auto it = g->rows_graphs.find(rows);
  if (rows <= 0 || it == g->rows_graphs.end()) return ctts_gpt_graph_launch(g, n_steps, stream);
  CttsDeviceGuard dg(stream);
  int left = n_steps;
  while (it->second.exec_multi && left >= g->multi_steps) { CK(hipGraphLaunch(it->second.exec_multi, (hipStream_t)stream)); left -= g->multi_steps; }
  for (int i = 0; i < left; ++i) CK(hipGraphLaunch(it->second.exec, (hipStream_t)stream));
  return 0;
}

extern "C" int ctts_gpt_profile_begin(ctts_gpt* g, int32_t tag, int32_t max_samples, int32_t stride) {
  if (!g || max_samples <= 0 || stride <= 0) return fail("bad profile args");
  while ((int)g->ev0.size() < max_samples) {
    hipEvent_t a, b;
    // hipEventDisableSystemFence: a default event makes the dispatch that signals it end with a system-scope release (L2
    // write-back towards the host) -- time that rocprofv3's own completion signals do not add to a kernel
    static int sysfence = -1;
    if (sysfence < 0) { const char* e = getenv("CTTS_PROF_SYSFENCE"); sysfence = (e && atoi(e) == 1) ? 1 : 0; }
    const unsigned fl = sysfence ? hipEventDefault : hipEventDisableSystemFence;
    CK(hipEventCreateWithFlags(&a, fl));
    CK(hipEventCreateWithFlags(&b, fl));
    g->ev0.push_back(a);
    g->ev1.push_back(b);
  }
  g->prof_tag = tag; g->prof_max = max_samples; g->prof_n = 0; g->prof_stride = stride; g->prof_seen = 0;
  return 0;
}

extern "C" int ctts_gpt_profile_samples(ctts_gpt* g, float* ms_out, int32_t cap, int32_t* n_samples) {
  if (!g || !ms_out || cap < 0) return fail("bad profile_samples args");
  const int n = g->prof_n < cap ? g->prof_n : cap;
  for (int i = 0; i < n; ++i) {
    CK(hipEventSynchronize(g->ev1[i]));
    CK(hipEventElapsedTime(&ms_out[i], g->ev0[i], g->ev1[i]));
  }
  if (n_samples) *n_samples = n;
  return 0;
}

extern "C" int ctts_gpt_profile_end(ctts_gpt* g, int32_t* n_samples, double* total_ms) {
  if (!g) return fail("null engine");
  double tot = 0.0;
  for (int i = 0; i < g->prof_n; ++i) {
    CK(hipEventSynchronize(g->ev1[i]));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, g->ev0[i], g->ev1[i]));
    tot += ms;
  }
  if (n_samples) *n_samples = g->prof_n;
  if (total_ms) *total_ms = tot;
  g->prof_tag = -1; g->prof_n = 0;
  return 0;
}

// ------------------------------------------------------------------------------------------------
struct ctts_codec {
  ctts_codec_weights w;
  std::vector<const float*> d[9], v[9];
  std::vector<const void*> dx[2], vx[2];   // pwconv1 / pwconv2 as pre-split fragment-order planes (codec_gemm.hip), or empty
  int x3p_min_rows = 1024;                 // frames from which the point-wise layers take the LDS-DMA kernel (env CTTS_X3P_MIN_ROWS, 0 = never).
                                           // Round 4: 12288 -> 1024 -- the first streamed window of a batch (64 x 144 = 9216 frames; 16 x 144 = 2304)
                                           // was on the register-staged tiles: TTFS p50 55.3 -> 50.4 ms at batch 64, 44.4 -> 40.1 ms at batch 16,
                                           // C5 total 252.7 -> 239.4 ms (profiles/r4o_ab_x3p_min_rows.log; 256 measures the same as 1024)
};

extern "C" int ctts_codec_create(ctts_codec** out, const ctts_codec_weights* w) {
  if (!out || !w) return fail("ctts_codec_create: bad arguments");
  ctts_codec* c = new ctts_codec();
  c->w = *w;
  const float* const* dsrc[9] = {w->d_dw_w, w->d_dw_b, w->d_ln_w, w->d_ln_b, w->d_pw1_w, w->d_pw1_b, w->d_pw2_w, w->d_pw2_b, w->d_gamma};
  const float* const* vsrc[9] = {w->v_dw_w, w->v_dw_b, w->v_ln_w, w->v_ln_b, w->v_pw1_w, w->v_pw1_b, w->v_pw2_w, w->v_pw2_b, w->v_gamma};
  for (int i = 0; i < 9; ++i) {
    c->d[i].assign(dsrc[i], dsrc[i] + w->n_dvae_blocks);
    c->v[i].assign(vsrc[i], vsrc[i] + w->n_vocos_blocks);
  }
  if (w->gemm_mode != 0 && w->gemm_mode != 1 && w->gemm_mode != 2) { delete c; return fail("ctts_codec_create: gemm_mode must be 0, 1 or 2"); }
  if (w->gemm_mode == 2 && !(w->d_pw1_x3p && w->d_pw2_x3p && w->v_pw1_x3p && w->v_pw2_x3p)) {
    delete c;
    return fail("ctts_codec_create: gemm_mode 2 needs the fp16 planes of the point-wise weights");
  }
  if (w->gemm_mode >= 1 && w->d_pw1_x3p && w->d_pw2_x3p && w->v_pw1_x3p && w->v_pw2_x3p) {
    c->dx[0].assign(w->d_pw1_x3p, w->d_pw1_x3p + w->n_dvae_blocks);
    c->dx[1].assign(w->d_pw2_x3p, w->d_pw2_x3p + w->n_dvae_blocks);
    c->vx[0].assign(w->v_pw1_x3p, w->v_pw1_x3p + w->n_vocos_blocks);
    c->vx[1].assign(w->v_pw2_x3p, w->v_pw2_x3p + w->n_vocos_blocks);
  }
  { const char* e = getenv("CTTS_X3P_MIN_ROWS"); if (e) c->x3p_min_rows = atoi(e); }
  *out = c;
  return 0;
}
extern "C" void ctts_codec_destroy(ctts_codec* c) { delete c; }

struct CodecWs {
  float *a, *b, *big, *mid, *frames;
  size_t bytes;
};
static CodecWs carve_codec(void* base, int B, int F) {
  const size_t R = ((size_t)B * F + 255) / 256 * 256;   // whole 256-row tiles: the packed planes of codec_gemm.hip are padded to them
  CodecWs w;
  size_t off = 0;
  char* p = (char*)base;
  w.a = (float*)(p + off); off += align_up(R * 512 * 4);
  w.b = (float*)(p + off); off += align_up(R * 512 * 4);
  w.big = (float*)(p + off); off += align_up(R * 2048 * 4);
  w.mid = (float*)(p + off); off += align_up(R * 384 * 4);
  w.frames = (float*)(p + off); off += align_up(R * 1024 * 4);
  w.bytes = off;
  return w;
}
extern "C" size_t ctts_codec_workspace_bytes(int32_t B, int32_t F) { return carve_codec(nullptr, B, F).bytes; }

static GemmArgs lin(const float* A, int lda, const float* W, float* C, int ldc, int M, int N, int K, int epi) {
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.lda = lda; a.W = W; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.wt = WT_F32; a.epi = epi; a.taps = 1;
  return a;
}
// dense layer of the decoder: f32 MFMA tiles, or split-bf16 tiles when the weights were packed [N][Kp/32][2][32] bf16
static hipError_t dense(const ctts_codec* c, const GemmArgs& a, hipStream_t st);
// seg != null: B = 1, the F frames are packed segments and the gather stays inside each row's own segment (ragged decode)
static GemmArgs conv(const float* X, int cin, const float* W, float* C, int cout, int B, int F, int taps, int pad, int epi, const int2* seg) {
  GemmArgs a = lin(X, cin, W, C, cout, B * F, cout, taps * cin, epi);
  a.taps = taps; a.cin = cin; a.frames = F; a.pad = pad; a.dil = 1; a.seg = seg;
  return a;
}

static int convnext_stack(const ctts_codec* c, int n, const std::vector<const float*>* p, const std::vector<const void*>* px, int inter, int dil,
                          CodecWs& ws, int B, int F, hipStream_t st, const int2* seg) {
  const int R = B * F;
  const bool f16 = c->w.gemm_mode == 2;   // one fp16 plane per operand (gemm_h1p_k) instead of hi | lo bf16 planes (gemm_x3p_k)
  const bool x3p = c->w.gemm_mode >= 1 && !px[0].empty() && c->x3p_min_rows > 0 && R >= c->x3p_min_rows && inter % 256 == 0;
  for (int i = 0; x3p && i < n; ++i) {
    // depthwise conv + LayerNorm -> bf16 planes; pwconv1 + GELU -> bf16 planes; pwconv2 * gamma + residual -> f32 rows
    uint16_t* bp = reinterpret_cast<uint16_t*>(ws.b);     // [R256][512] as hi / lo planes: the bytes of the f32 buffer
    uint16_t* bigp = reinterpret_cast<uint16_t*>(ws.big);
    CK(launch_dwconv_ln(ws.a, p[0][i], p[1][i], p[2][i], p[3][i], 1e-6f, dil, nullptr, B, F, 512, st, bp, f16 ? 1 : 0, seg));
    if (f16 && mlp_fused_pays(R)) {   // round 6: the pair in one launch, the inter-wide activation stays on the CU (bit-identical)
      MlpArgs m;
      memset(&m, 0, sizeof(m));
      m.Ap = bp; m.W1p = (const uint16_t*)px[0][i]; m.W2p = (const uint16_t*)px[1][i]; m.M = R; m.inter = inter;
      m.b1 = p[5][i]; m.b2 = p[7][i]; m.gamma = p[8][i]; m.C = ws.a;
      CK(launch_mlp_fused_h1p(m, st));
      continue;
    }
    X3pArgs g;
    memset(&g, 0, sizeof(g));
    g.Ap = bp; g.Wp = (const uint16_t*)px[0][i]; g.M = R; g.N = inter; g.K = 512; g.epi = X3P_GELU_PACKED; g.bias = p[5][i]; g.Cp = bigp;
    CK(f16 ? launch_gemm_h1p(g, st) : launch_gemm_x3p(g, st));
    g.Ap = bigp; g.Wp = (const uint16_t*)px[1][i]; g.N = 512; g.K = inter; g.epi = X3P_SCALE_RES; g.bias = p[7][i]; g.gamma = p[8][i];
    g.res = ws.a; g.ldr = 512; g.C = ws.a; g.ldc = 512; g.Cp = nullptr;
    CK(f16 ? launch_gemm_h1p(g, st) : launch_gemm_x3p(g, st));
  }
  for (int i = 0; !x3p && i < n; ++i) {
    CK(launch_dwconv_ln(ws.a, p[0][i], p[1][i], p[2][i], p[3][i], 1e-6f, dil, ws.b, B, F, 512, st, nullptr, 0, seg));
    GemmArgs g1 = lin(ws.b, 512, p[4][i], ws.big, inter, R, inter, 512, EPI_BIAS_GELU);
    g1.bias = p[5][i];
    CK(dense(c, g1, st));
    GemmArgs g2 = lin(ws.big, inter, p[6][i], ws.a, 512, R, 512, inter, EPI_BIAS_SCALE_RES);
    g2.bias = p[7][i]; g2.gamma = p[8][i]; g2.res = ws.a; g2.ldr = 512;
    CK(dense(c, g2, st));
  }
  return 0;
}

static hipError_t dense(const ctts_codec* c, const GemmArgs& a, hipStream_t st) {
  return c->w.gemm_mode >= 1 ? launch_gemm_tiled_bf16x3(a, st) : launch_gemm_tiled(a, st);   // mode 2: only the ConvNeXt point-wise pairs are fp16
}

// the decoder bodies: [B, F] batches (seg null) or B = 1 packed segments (seg = the per-frame bounds table, ragged decode)
static int dvae_body(ctts_codec* c, const float* hid, float* mel, int B, int F, CodecWs& ws, const int2* seg, hipStream_t st) {
  // dvae.py:281-287: [B,T,768] viewed as [B,2T,384] channels-last
  GemmArgs c0 = conv(hid, 384, c->w.conv_in0_w, ws.big, 128, B, F, 3, 1, EPI_BIAS_GELU, seg);
  c0.bias = c->w.conv_in0_b;
  CK(dense(c, c0, st));
  GemmArgs c2 = conv(ws.big, 128, c->w.conv_in2_w, ws.a, 512, B, F, 3, 1, EPI_BIAS, seg);
  c2.bias = c->w.conv_in2_b;
  CK(dense(c, c2, st));
  if (convnext_stack(c, c->w.n_dvae_blocks, c->d, c->dx, 2048, 2, ws, B, F, st, seg)) return -1;
  CK(dense(c, lin(ws.a, 512, c->w.conv_out_w, ws.mid, 384, B * F, 384, 512, EPI_STORE), st));
  GemmArgs oc = conv(ws.mid, 384, c->w.out_conv_w, mel, 100, B, F, 3, 1, EPI_SCALE, seg);
  oc.gamma = c->w.coef;
  CK(dense(c, oc, st));
  return 0;
}

static int vocos_body(ctts_codec* c, const float* mel, int B, int F, CodecWs& ws, const int2* seg, hipStream_t st) {   // -> ws.big: the head
  GemmArgs e = conv(mel, 100, c->w.v_embed_w, ws.b, 512, B, F, 7, 3, EPI_BIAS, seg);
  e.bias = c->w.v_embed_b;
  CK(dense(c, e, st));
  CK(launch_layernorm(ws.b, c->w.v_norm_w, c->w.v_norm_b, 1e-6f, ws.a, B * F, 512, st));
  if (convnext_stack(c, c->w.n_vocos_blocks, c->v, c->vx, 1536, 1, ws, B, F, st, seg)) return -1;
  CK(launch_layernorm(ws.a, c->w.v_final_w, c->w.v_final_b, 1e-6f, ws.b, B * F, 512, st));
  GemmArgs h = lin(ws.b, 512, c->w.head_w, ws.big, 1026, B * F, 1026, 512, EPI_BIAS);
  h.bias = c->w.head_b;
  CK(dense(c, h, st));
  return 0;
}

extern "C" int ctts_dvae_decode(ctts_codec* c, const float* hid, float* mel, int32_t B, int32_t T, void* workspace, size_t ws_bytes,
                                void* stream) {
  if (!c || B <= 0 || T <= 0) return fail("ctts_dvae_decode: bad arguments");
  CttsDeviceGuard dg(stream);
  const int F = 2 * T;
  if (ws_bytes < ctts_codec_workspace_bytes(B, F)) return fail("codec workspace too small");
  CodecWs ws = carve_codec(workspace, B, F);
  return dvae_body(c, hid, mel, B, F, ws, nullptr, (hipStream_t)stream);
}

extern "C" int ctts_vocos_decode(ctts_codec* c, const float* mel, float* wav, int32_t B, int32_t F, void* workspace, size_t ws_bytes,
                                 void* stream) {
  if (!c || B <= 0 || F < 2) return fail("ctts_vocos_decode: bad arguments");
  CttsDeviceGuard dg(stream);
  if (ws_bytes < ctts_codec_workspace_bytes(B, F)) return fail("codec workspace too small");
  hipStream_t st = (hipStream_t)stream;
  CodecWs ws = carve_codec(workspace, B, F);
  if (vocos_body(c, mel, B, F, ws, nullptr, st)) return -1;
  CK(launch_istft(ws.big, c->w.window, c->w.twiddle, ws.frames, wav, B, F, st));
  return 0;
}

// ---- ragged decode: packed segments, each decoded as if alone ---------------------------------------------------------------
// workspace = the [1, sum F_i] codec workspace + the per-frame segment bounds table behind it
static size_t ragged_table_offset(int total_tokens) { return carve_codec(nullptr, 1, 2 * total_tokens).bytes; }
extern "C" size_t ctts_codec_ragged_workspace_bytes(int32_t n_seg, int32_t total_tokens) {
  if (n_seg < 1 || total_tokens < n_seg) return 0;
  return ragged_table_offset(total_tokens) + align_up((size_t)2 * total_tokens * sizeof(int2));
}
// token offsets (host copy): offs[0] = 0, strictly ascending (no empty segment); returns the total and the longest segment, or -1
static int check_offsets(const char* who, const int32_t* offs, int n_seg, int* t_max) {
  if (!offs || n_seg < 1) return fail("%s: need n_seg >= 1 and the host offsets", who);
  if (offs[0] != 0) return fail("%s: the first token offset must be 0 (got %d)", who, offs[0]);
  int mx = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (offs[i + 1] <= offs[i]) return fail("%s: segment %d is empty or the offsets do not ascend (%d -> %d)", who, i, offs[i], offs[i + 1]);
    if (offs[i + 1] > (1 << 28)) return fail("%s: too many tokens", who);
    mx = std::max(mx, offs[i + 1] - offs[i]);
  }
  *t_max = mx;
  return offs[n_seg];
}

extern "C" int ctts_dvae_decode_ragged(ctts_codec* c, const float* hid, const int32_t* tok_off_dev, const int32_t* tok_off_host, int32_t n_seg,
                                       float* mel, void* workspace, size_t ws_bytes, void* stream) {
  if (!c || !hid || !mel || !tok_off_dev) return fail("ctts_dvae_decode_ragged: bad arguments");
  int t_max = 0;
  const int T = check_offsets("ctts_dvae_decode_ragged", tok_off_host, n_seg, &t_max);
  if (T < 0) return -1;
  if (!workspace || ws_bytes < ctts_codec_ragged_workspace_bytes(n_seg, T)) return fail("codec workspace too small");
  CttsDeviceGuard dg(stream);
  hipStream_t st = (hipStream_t)stream;
  const int F = 2 * T;
  CodecWs ws = carve_codec(workspace, 1, F);
  int2* seg = (int2*)((char*)workspace + ragged_table_offset(T));
  CK(launch_segment_table(tok_off_dev, n_seg, seg, st));
  return dvae_body(c, hid, mel, 1, F, ws, seg, st);
}

extern "C" int ctts_vocos_decode_ragged(ctts_codec* c, const float* mel, const int32_t* tok_off_dev, const int32_t* tok_off_host, int32_t n_seg,
                                        float* wav, void* workspace, size_t ws_bytes, void* stream) {
  if (!c || !mel || !wav || !tok_off_dev) return fail("ctts_vocos_decode_ragged: bad arguments");
  int t_max = 0;
  const int T = check_offsets("ctts_vocos_decode_ragged", tok_off_host, n_seg, &t_max);
  if (T < 0) return -1;
  if (!workspace || ws_bytes < ctts_codec_ragged_workspace_bytes(n_seg, T)) return fail("codec workspace too small");
  CttsDeviceGuard dg(stream);
  hipStream_t st = (hipStream_t)stream;
  const int F = 2 * T;
  CodecWs ws = carve_codec(workspace, 1, F);
  int2* seg = (int2*)((char*)workspace + ragged_table_offset(T));
  CK(launch_segment_table(tok_off_dev, n_seg, seg, st));
  if (vocos_body(c, mel, 1, F, ws, seg, st)) return -1;
  CK(launch_istft_ragged(ws.big, c->w.window, c->w.twiddle, ws.frames, wav, tok_off_dev, n_seg, F, 2 * t_max, st));
  return 0;
}

// ---- window decode: the due chunks of many streams in one ragged pass, each window at its own position of its own slot ----------------
static_assert(sizeof(ctts_window) == 32 && sizeof(CodecWindow) == 32 && offsetof(ctts_window, keep) == offsetof(CodecWindow, keep) &&
              offsetof(ctts_window, c_lo) == offsetof(CodecWindow, c_lo), "ctts_window layout");
// workspace = the ragged workspace | packed hidden rows [T, 768] | tok_off [n_win + 1] | mel [2 T, 100] | wav [256 (2 T - n_win)]
struct WindowsWs {
  float *hid, *mel, *wav;
  int32_t* tok_off;
  size_t ragged_bytes, bytes;
};
static WindowsWs carve_windows(void* base, int n_win, int T) {
  WindowsWs w;
  char* p = (char*)base;
  size_t off = w.ragged_bytes = ctts_codec_ragged_workspace_bytes(n_win, T);
  w.hid = (float*)(p + off); off += align_up((size_t)T * 768 * 4);
  w.tok_off = (int32_t*)(p + off); off += align_up((size_t)(n_win + 1) * 4);
  w.mel = (float*)(p + off); off += align_up((size_t)2 * T * 100 * 4);
  w.wav = (float*)(p + off); off += align_up((size_t)256 * (2 * (size_t)T - n_win) * 4);
  w.bytes = off;
  return w;
}
extern "C" size_t ctts_codec_windows_workspace_bytes(int32_t n_win, int32_t total_tokens) {
  if (n_win < 1 || total_tokens < n_win || ctts_codec_ragged_workspace_bytes(n_win, total_tokens) == 0) return 0;
  return carve_windows(nullptr, n_win, total_tokens).bytes;
}
// -- what the three entries below share: the checks of the host mirror and the front half, up to the packed waveforms -------------------
static int check_out_format(const char* who, int out_type, int product, const void* out) {
  if ((out_type != 0 && out_type != 1) || (product != 0 && product != 1)) return fail("%s: out_type and product must be 0 or 1", who);
  if ((uintptr_t)out & 15) return fail("%s: the output must be 16-byte aligned", who);
  return 0;
}
static int check_store(const char* who, const float* hid, int64_t slot_stride, int64_t row_stride, int n_slots, int hid_cap) {
  if (n_slots < 1 || hid_cap < 1 || row_stride < 768 || slot_stride < (int64_t)hid_cap * row_stride || (row_stride & 3) || (slot_stride & 3) ||
      ((uintptr_t)hid & 15))
    return fail("%s: the store must be [n_slots][hid_cap][768] floats with 16-byte aligned rows", who);
  return 0;
}
// the windows of the host mirror: slot, token range, capacity, crop -- everything the gather and the crop trust.  Fills tok[0 .. n_win],
// the windows' token offsets in the packed decode
static int check_windows(const char* who, const ctts_window* win_host, int n_win, int n_slots, int hid_cap, std::vector<int32_t>& tok) {
  tok.assign(n_win + 1, 0);
  for (int i = 0; i < n_win; ++i) {
    const ctts_window& w = win_host[i];
    if (w.slot < 0 || w.slot >= n_slots) return fail("%s: window %d names slot %d of %d", who, i, w.slot, n_slots);
    if (w.t_lo < 0 || w.t_hi <= w.t_lo) return fail("%s: window %d is empty (tokens %d -> %d)", who, i, w.t_lo, w.t_hi);
    if (w.t_hi > hid_cap) return fail("%s: window %d ends at token %d beyond the slot's capacity %d", who, i, w.t_hi, hid_cap);
    const int64_t n_samples = 256 * (2 * (int64_t)(w.t_hi - w.t_lo) - 1);
    if (w.c_lo < 0 || w.c_hi <= w.c_lo || w.c_hi > n_samples)
      return fail("%s: window %d crops samples %d -> %d outside its %lld samples", who, i, w.c_lo, w.c_hi, (long long)n_samples);
    tok[i + 1] = tok[i] + (w.t_hi - w.t_lo);
    if (tok[i + 1] > (1 << 28)) return fail("%s: too many tokens", who);
  }
  return 0;
}
// gather -> DVAE -> Vocos over the checked table: every window is a ragged segment, its edges are sequence edges.  Leaves ws.wav filled
static int decode_windows_front(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, const ctts_window* win_dev, int n_win,
                                const std::vector<int32_t>& tok, const WindowsWs& ws, void* workspace, void* stream) {
  {
    CttsDeviceGuard dg(stream);
    CK(launch_gather_windows(hid, slot_stride, row_stride, (const CodecWindow*)win_dev, n_win, tok[n_win], ws.hid, ws.tok_off, (hipStream_t)stream));
  }
  if (ctts_dvae_decode_ragged(c, ws.hid, ws.tok_off, tok.data(), n_win, ws.mel, workspace, ws.ragged_bytes, stream)) return -1;
  return ctts_vocos_decode_ragged(c, ws.mel, ws.tok_off, tok.data(), n_win, ws.wav, workspace, ws.ragged_bytes, stream);
}

extern "C" int ctts_codec_decode_windows(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots, int32_t hid_cap,
                                         const ctts_window* win_dev, const ctts_window* win_host, int32_t n_win, int32_t out_type, void* out,
                                         uint8_t* keep_bits, int32_t product, float keep_thr, void* workspace, size_t ws_bytes, void* stream) {
  const char* who = "ctts_codec_decode_windows";
  if (!c || !hid || !win_dev || !win_host || !out) return fail("%s: bad arguments", who);
  if (n_win < 1 || n_win > 1024) return fail("%s: need 1 <= n_win <= 1024 (got %d)", who, n_win);
  if (check_out_format(who, out_type, product, out) || check_store(who, hid, slot_stride, row_stride, n_slots, hid_cap)) return -1;
  std::vector<int32_t> tok;
  if (check_windows(who, win_host, n_win, n_slots, hid_cap, tok)) return -1;
  for (int i = 0; i < n_win; ++i)
    if (win_host[i].keep && !keep_bits) return fail("%s: window %d asks for a keep mask but keep_bits is null", who, i);
  const int T = tok[n_win];
  if (!workspace || ws_bytes < ctts_codec_windows_workspace_bytes(n_win, T)) return fail("codec workspace too small");
  WindowsWs ws = carve_windows(workspace, n_win, T);
  if (decode_windows_front(c, hid, slot_stride, row_stride, win_dev, n_win, tok, ws, workspace, stream)) return -1;
  CttsDeviceGuard dg(stream);
  CK(launch_crop_pcm16_windows(ws.wav, (const CodecWindow*)win_dev, n_win, out_type == 0 ? 1 : 0, product, keep_thr, out, keep_bits,
                               (hipStream_t)stream));
  return 0;
}

// ---- window decode at other sample rates: the windows' chunks are outputs [o_lo, o_hi) of the resampled prefix ------------------------
static_assert(sizeof(ctts_rs_window) == 64 && sizeof(RsWindow) == 64 && offsetof(ctts_rs_window, out_off) == offsetof(RsWindow, out_off) &&
              offsetof(ctts_rs_window, rate) == offsetof(RsWindow, rate) && offsetof(ctts_rs_window, pad) == offsetof(RsWindow, pad),
              "ctts_rs_window layout");
// the inputs inside [0, total) that outputs [o_lo, o_hi) read (resample.py, window_inputs) must lie in the window; everything in the host
// mirror that a launch would trust.  o_lo == o_hi (an empty chunk) reads nothing
static int check_rs_window(const char* who, int i, const ctts_rs_window& w, int L, int M, int K) {
  if (w.o_lo < 0 || w.o_hi < w.o_lo) return fail("%s: window %d wants outputs %lld -> %lld", who, i, (long long)w.o_lo, (long long)w.o_hi);
  if (w.n_in < 1 || w.in_off < 0 || w.origin < 0 || w.total < 1 || w.origin + w.n_in > w.total || w.total >= (1ll << 31))
    return fail("%s: window %d holds samples %lld + %lld of a signal of %lld", who, i, (long long)w.origin, (long long)w.n_in, (long long)w.total);
  if (w.o_hi > (w.total * L + M - 1) / M)
    return fail("%s: window %d ends at output %lld beyond the signal's ceil(total L / M)", who, i, (long long)w.o_hi);
  if (w.out_off < 0 || w.pad < 0 || w.pad > 255) return fail("%s: window %d: bad output offset or pad", who, i);
  if (w.o_hi == w.o_lo) return 0;
  const long long width = (K - M) / 2;
  const long long a = std::max(0ll, (long long)(w.o_lo / L) * M - width), b = std::min((long long)w.total, (long long)((w.o_hi - 1) / L) * M + width + M);
  if (a < b && (w.origin > a || w.origin + w.n_in < b))
    return fail("%s: window %d holds samples [%lld, %lld) but its outputs read [%lld, %lld)", who, i, (long long)w.origin,
                (long long)(w.origin + w.n_in), a, b);
  return 0;
}
static int check_rs_pair(const char* who, const float* taps, int L, int M, int K) {
  if (!taps) return fail("%s: the filter table is null", who);
  if (L < 1 || M < 1 || L == M) return fail("%s: need L != M, both positive (got %d/%d)", who, L, M);
  if (resample_mode(L, M, K) == 0)
    return fail("%s: conversion %d/%d with %d taps is not supported (K = 2 width + M; a tile's input span within %d floats, the table within %d)",
                who, L, M, K, RS_LDS_FLOATS, RS_TAB_MAX);
  return 0;
}
extern "C" int ctts_resample_windows(const float* x, int64_t n_x, const ctts_rs_window* win_dev, const ctts_rs_window* win_host, int32_t n_win,
                                     float* y, int64_t n_y, const int32_t* sel_dev, const int32_t* sel_host, int32_t n_sel, const float* taps,
                                     int32_t L, int32_t M, int32_t K, void* stream) {
  const char* who = "ctts_resample_windows";
  if (!x || !y || !win_dev || !win_host) return fail("%s: bad arguments", who);
  if (n_win < 1 || n_win > 1024) return fail("%s: need 1 <= n_win <= 1024 (got %d)", who, n_win);
  if ((sel_dev == nullptr) != (sel_host == nullptr)) return fail("%s: the window selection must be given on the device and the host, or on neither", who);
  if (check_rs_pair(who, taps, L, M, K)) return -1;
  const int n_launch = sel_host ? n_sel : n_win;
  if (n_launch < 1 || n_launch > 1024) return fail("%s: need 1 <= converted windows <= 1024 (got %d)", who, n_launch);
  long long n_out_max = 0;
  for (int q = 0; q < n_launch; ++q) {
    const int i = sel_host ? sel_host[q] : q;
    if (i < 0 || i >= n_win) return fail("%s: selected window %d is outside the table", who, i);
    const ctts_rs_window& w = win_host[i];
    if (check_rs_window(who, i, w, L, M, K)) return -1;
    if (w.in_off + w.n_in > n_x || w.out_off + (w.o_hi - w.o_lo) + w.pad > n_y)
      return fail("%s: window %d lies outside the input (%lld floats) or the output (%lld floats)", who, i, (long long)n_x, (long long)n_y);
    n_out_max = std::max(n_out_max, (long long)(w.o_hi - w.o_lo));
  }
  CttsDeviceGuard dg(stream);
  CK(launch_resample_windows(x, (const RsWindow*)win_dev, y, sel_dev, n_launch, n_out_max, taps, L, M, K, (hipStream_t)stream));
  return 0;
}

// workspace = the window-decode workspace | the resampled chunks, chunk_floats of them (sum of ceil8(o_hi - o_lo) over the resampled windows)
extern "C" size_t ctts_codec_windows_rate_workspace_bytes(int32_t n_win, int32_t total_tokens, int64_t chunk_floats) {
  const size_t base = ctts_codec_windows_workspace_bytes(n_win, total_tokens);
  if (base == 0 || chunk_floats < 0 || chunk_floats >= (1ll << 31)) return 0;
  return base + align_up((size_t)chunk_floats * 4);
}
extern "C" int ctts_codec_decode_windows_rate(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots,
                                              int32_t hid_cap, const ctts_window* win_dev, const ctts_window* win_host,
                                              const ctts_rs_window* rs_dev, const ctts_rs_window* rs_host, const int32_t* sel_dev, const int32_t* sel_host,
                                              int32_t n_win,
                                              const ctts_rate* rates, int32_t n_rates, int32_t out_type, void* out, uint8_t* keep_bits,
                                              int32_t product, float keep_thr, void* workspace, size_t ws_bytes, void* stream) {
  const char* who = "ctts_codec_decode_windows_rate";
  if (!c || !hid || !win_dev || !win_host || !rs_dev || !rs_host || !sel_dev || !sel_host || !out) return fail("%s: bad arguments", who);
  if (n_win < 1 || n_win > 1024) return fail("%s: need 1 <= n_win <= 1024 (got %d)", who, n_win);
  if (n_rates < 0 || n_rates > n_win || (n_rates > 0 && !rates)) return fail("%s: need 0 <= n_rates <= n_win and the rate table", who);
  if (check_out_format(who, out_type, product, out) || check_store(who, hid, slot_stride, row_stride, n_slots, hid_cap)) return -1;
  for (int r = 0; r < n_rates; ++r)
    if (check_rs_pair(who, rates[r].taps, rates[r].L, rates[r].M, rates[r].K)) return -1;
  std::vector<int32_t> tok;
  if (check_windows(who, win_host, n_win, n_slots, hid_cap, tok)) return -1;
  std::vector<int> per_rate(n_rates, 0);
  std::vector<long long> longest(n_rates, 0);
  long long chunk_floats = 0;
  for (int i = 0; i < n_win; ++i) {
    const ctts_window& w = win_host[i];
    const ctts_rs_window& r = rs_host[i];
    if (w.keep && !keep_bits) return fail("%s: window %d asks for a keep mask but keep_bits is null", who, i);
    const int64_t start = 256 * (2 * (int64_t)tok[i] - i);       // the window's first sample in the packed decode
    if (r.rate >= n_rates) return fail("%s: window %d names rate %d of %d", who, i, r.rate, n_rates);
    if (r.rate < 0) {                                            // stays at 24 kHz: the crop itself
      if (r.in_off != start + w.c_lo || r.n_in != w.c_hi - w.c_lo) return fail("%s: window %d: the 24 kHz chunk is not the window's crop", who, i);
    } else {
      // the resampler reads the crop alone: samples [origin, origin + n_in) = [512 t_lo + c_lo, 512 t_lo + c_hi) of the prefix
      if (r.in_off != start + w.c_lo || r.n_in != w.c_hi - w.c_lo || r.origin != 512 * (int64_t)w.t_lo + w.c_lo)
        return fail("%s: window %d: the resampler's input is not the window's crop at its place in the prefix", who, i);
      if (r.o_hi <= r.o_lo) return fail("%s: window %d wants outputs %lld -> %lld", who, i, (long long)r.o_lo, (long long)r.o_hi);
      if (check_rs_window(who, i, r, rates[r.rate].L, rates[r.rate].M, rates[r.rate].K)) return -1;
      const long long n = r.o_hi - r.o_lo;
      if (r.out_off != chunk_floats || r.pad != (int)(((n + 7) & ~7ll) - n)) return fail("%s: window %d: chunks start on multiples of 8 floats, zero padded", who, i);
      chunk_floats += n + r.pad;
      ++per_rate[r.rate];
      longest[r.rate] = std::max(longest[r.rate], n);
    }
  }
  // sel lists the resampled windows rate by rate, each once: one launch per distinct rate converts its run of the list
  for (int r = 0, q = 0; r < n_rates; ++r)
    for (int k = 0; k < per_rate[r]; ++k, ++q) {
      const int i = sel_host[q];
      if (i < 0 || i >= n_win || rs_host[i].rate != r || (k > 0 && i <= sel_host[q - 1]))
        return fail("%s: the selection must list the resampled windows rate by rate, ascending within a rate", who);
    }
  const int T = tok[n_win];
  if (!workspace || ws_bytes < ctts_codec_windows_rate_workspace_bytes(n_win, T, chunk_floats) || chunk_floats >= (1ll << 31))
    return fail("codec workspace too small");
  WindowsWs ws = carve_windows(workspace, n_win, T);
  float* chunks = (float*)((char*)workspace + ws.bytes);
  if (decode_windows_front(c, hid, slot_stride, row_stride, win_dev, n_win, tok, ws, workspace, stream)) return -1;
  CttsDeviceGuard dg(stream);
  int done = 0;
  for (int r = 0; r < n_rates; ++r) {
    CK(launch_resample_windows(ws.wav, (const RsWindow*)rs_dev, chunks, sel_dev + done, per_rate[r], longest[r], rates[r].taps, rates[r].L,
                               rates[r].M, rates[r].K, (hipStream_t)stream));
    done += per_rate[r];
  }
  CK(launch_chunks_pcm16(ws.wav, chunks, (const CodecWindow*)win_dev, (const RsWindow*)rs_dev, n_win, out_type == 0 ? 1 : 0, product, keep_thr,
                         out, keep_bits, (hipStream_t)stream));
  return 0;
}

// ---- time scaling of streams: the host's arithmetic (timescale.py: a_of, need, frames_final, base) and every check a launch trusts -------
static_assert(sizeof(ctts_ts_stream) == 80 && sizeof(TsStream) == 80 && offsetof(ctts_ts_stream, k_prev) == offsetof(TsStream, k_prev) &&
              offsetof(ctts_ts_stream, slot) == offsetof(TsStream, slot) && offsetof(ctts_ts_stream, n_out) == offsetof(TsStream, n_out) &&
              CTTS_TS_CARRY == TS_CARRY && CTTS_TS_STATE_INTS == TS_STATE_INTS, "ctts_ts_stream layout");
static long long ts_a(long long k, long long num) { return k * TS_HS * num / 100; }
static long long ts_need(long long k, long long num) {
  return k < 1 ? 0 : std::max(ts_a(k - 1, num) + TS_D + TS_N - 1, ts_a(k, num) - TS_HS + TS_D + TS_N - 1);
}
static long long ts_frames_final(long long n_avail, long long num) {
  long long k = n_avail * 100 / (TS_HS * num) + 2;   // need(k) > k HS num / den: above every frame that may run
  while (k > 0 && ts_need(k, num) > n_avail) --k;
  return k;
}
static long long ts_base(long long k, long long num) { return std::max(0ll, ts_a(k, num) - TS_HS - TS_D); }
static long long ts_path_entries(const ctts_ts_stream& w) { return (long long)w.k_now - w.k_prev + (w.k_prev == 0 && w.k_now > 0 ? 1 : 0); }
// streams [lo, hi) of the host mirror: one launch's worth.  `seen`: n_slots flags, cleared here
static int check_ts_streams(const char* who, const ctts_ts_stream* tab, int lo, int hi, long long n_x, long long n_y, long long n_path, int n_slots,
                            std::vector<char>& seen) {
  std::fill(seen.begin(), seen.end(), 0);
  for (int i = lo; i < hi; ++i) {
    const ctts_ts_stream& w = tab[i];
    if (w.den != 100 || w.num < 50 || w.num > 200) return fail("%s: stream %d: the speed is num / 100 with 50 <= num <= 200 (got %d/%d)", who, i, w.num, w.den);
    if (w.num == w.den) return fail("%s: stream %d: speed 1 (%d/%d): there is nothing to scale", who, i, w.num, w.den);
    if (w.slot < 0 || w.slot >= n_slots) return fail("%s: stream %d: slot %d is outside the pool of %d", who, i, w.slot, n_slots);
    if (seen[w.slot]) return fail("%s: stream %d: slot %d appears twice in one launch", who, i, w.slot);
    seen[w.slot] = 1;
    if (w.phase != 0 && w.phase != 1) return fail("%s: stream %d: phase %d is neither 0 nor 1", who, i, w.phase);
    if (w.n_in < 0 || w.pos < 0 || w.in_off < 0 || w.out_off < 0 || w.path_off < 0) return fail("%s: stream %d: a negative length, position or offset", who, i);
    if (w.pos >= (1ll << 31) || w.n_in >= (1ll << 31) || w.pos + w.n_in >= (1ll << 31) - 4096)
      return fail("%s: stream %d would hold 2^31 samples or more (less the 4096 a frame may reach past them)", who, i);
    if (w.in_off + w.n_in > n_x) return fail("%s: stream %d: the push lies outside the input (%lld floats)", who, i, n_x);
    const long long end = w.pos + w.n_in;
    const bool fin = w.total != -1;
    if (fin && (w.total != end || w.total < 1))
      return fail("%s: stream %d: a last push ends the stream at pos + n_in = %lld >= 1, got total %lld", who, i, end, (long long)w.total);
    const long long kp = ts_frames_final(w.pos, w.num);
    const long long m = (end * w.den + w.num - 1) / w.num;
    const long long kn = fin ? (m + TS_HS - 1) / TS_HS : ts_frames_final(end, w.num);
    if (w.k_prev != kp || w.k_now != kn)
      return fail("%s: stream %d: %lld + %lld samples at %d/%d make frames (%lld, %lld] final, got (%d, %d]", who, i, (long long)w.pos, (long long)w.n_in,
                  w.num, w.den, kp, kn, w.k_prev, w.k_now);
    const long long no = fin ? m - TS_HS * kp : TS_HS * (kn - kp);
    if (w.n_out != no) return fail("%s: stream %d: the step emits %lld samples, got %d", who, i, no, w.n_out);
    if (w.out_off + no > n_y) return fail("%s: stream %d: the chunk lies outside the output (%lld floats)", who, i, n_y);
    if (w.path_off + ts_path_entries(w) > n_path) return fail("%s: stream %d: the path entries lie outside the path (%lld entries)", who, i, n_path);
    const long long c_in = w.pos - ts_base(kp, w.num), c_out = fin ? 0 : end - ts_base(kn, w.num);
    if (c_in < 0 || c_in > TS_CARRY || c_out < 0 || c_out > TS_CARRY)
      return fail("%s: stream %d: a carry of %lld samples exceeds the %d a slot keeps", who, i, std::max(c_in, c_out), TS_CARRY);
  }
  return 0;
}
extern "C" int ctts_time_scale_stream_step(const float* x, int64_t n_x, const ctts_ts_stream* st_dev, const ctts_ts_stream* st_host,
                                           int32_t n_streams, float* y, int64_t n_y, int32_t* path, int64_t n_path, float* carry, int32_t* state,
                                           int32_t n_slots, const float* window, void* stream) {
  const char* who = "ctts_time_scale_stream_step";
  if (!st_dev || !st_host || !carry || !state || !window)
    return fail("%s: a null pointer (both descriptor tables, the carry, the state and the window are needed)", who);
  if (n_x < 0 || n_y < 0 || n_path < 0 || (!x && n_x) || (!y && n_y) || (!path && n_path))
    return fail("%s: a null pointer (x, y or path) with a length other than 0", who);
  if (n_streams < 1 || n_streams > 1024) return fail("%s: need 1 <= n_streams <= 1024 (got %d)", who, n_streams);
  if (n_slots < 1) return fail("%s: the state pool has no slot", who);
  std::vector<char> seen((size_t)n_slots, 0);
  if (check_ts_streams(who, st_host, 0, n_streams, n_x, n_y, n_path, n_slots, seen)) return -1;
  CttsDeviceGuard dg(stream);
  CK(launch_time_scale_stream(x, (const TsStream*)st_dev, n_streams, y, path, carry, state, window, (hipStream_t)stream));
  return 0;
}

// ---- sample-rate conversion of streams: the host's arithmetic (resample.py: stream_plan) and every check a launch trusts ---------------
static_assert(sizeof(ctts_rs_stream) == 80 && sizeof(RsStream) == 80 && offsetof(ctts_rs_stream, n_out) == offsetof(RsStream, n_out) &&
              offsetof(ctts_rs_stream, slot) == offsetof(RsStream, slot) && offsetof(ctts_rs_stream, c_out) == offsetof(RsStream, c_out) &&
              offsetof(ctts_rs_stream, pad) == offsetof(RsStream, pad) && CTTS_RS_CARRY == RS_CARRY, "ctts_rs_stream layout");
// the frames j whose inputs [j M - width, j M + width + M) lie within the first p samples
static long long rs_frames_final(long long p, long long M, long long width) { return p >= width + M ? (p - width - M) / M + 1 : 0; }
// descriptors [lo, hi) of the host mirror: one launch's worth, all by L/M/K.  `seen`: n_slots flags, cleared here; *n_out_max: the longest chunk
static int check_rs_streams(const char* who, const ctts_rs_stream* tab, int lo, int hi, long long n_x, long long n_y, int n_slots, int L, int M,
                            int K, std::vector<char>& seen, long long* n_out_max) {
  std::fill(seen.begin(), seen.end(), 0);
  const long long width = (K - M) / 2;
  *n_out_max = 0;
  for (int i = lo; i < hi; ++i) {
    const ctts_rs_stream& w = tab[i];
    if (w.slot < 0 || w.slot >= n_slots) return fail("%s: resampler stream %d: slot %d is outside the pool of %d", who, i, w.slot, n_slots);
    if (seen[w.slot]) return fail("%s: resampler stream %d: slot %d appears twice in one launch", who, i, w.slot);
    seen[w.slot] = 1;
    if (w.phase != 0 && w.phase != 1) return fail("%s: resampler stream %d: phase %d is neither 0 nor 1", who, i, w.phase);
    if (w.n_in < 0 || w.pos < 0 || w.in_off < 0 || w.out_off < 0 || w.o_lo < 0 || w.n_out < 0)
      return fail("%s: resampler stream %d: a negative length, position or offset", who, i);
    if (w.pad < 0 || w.pad > 255) return fail("%s: resampler stream %d: a pad of %d is outside 0 .. 255", who, i, w.pad);
    if (w.pos >= (1ll << 31) || w.n_in >= (1ll << 31) || w.pos + w.n_in >= (1ll << 31))
      return fail("%s: resampler stream %d would hold 2^31 samples or more", who, i);
    if (w.in_off + w.n_in > n_x) return fail("%s: resampler stream %d: the push lies outside the input (%lld floats)", who, i, n_x);
    const long long end = w.pos + w.n_in;
    const bool fin = w.total != -1;
    if (fin && (w.total != end || w.total < 1))
      return fail("%s: resampler stream %d: a last push ends the stream at pos + n_in = %lld >= 1, got total %lld", who, i, end, (long long)w.total);
    const long long e0 = rs_frames_final(w.pos, M, width) * L;
    if (w.o_lo != e0) return fail("%s: resampler stream %d: %lld samples have emitted %lld outputs, got o_lo %lld", who, i, (long long)w.pos, e0, (long long)w.o_lo);
    const long long e1 = fin ? (end * L + M - 1) / M : std::max(e0, rs_frames_final(end, M, width) * L);
    if (e1 >= (1ll << 31)) return fail("%s: resampler stream %d would emit 2^31 samples or more", who, i);
    if (w.n_out != e1 - e0) return fail("%s: resampler stream %d: the step emits %lld samples, got %lld", who, i, e1 - e0, (long long)w.n_out);
    if (w.out_off + w.n_out + w.pad > n_y) return fail("%s: resampler stream %d: the chunk lies outside the output (%lld floats)", who, i, n_y);
    const long long c_in = w.pos - std::max(0ll, (e0 / L) * M - width), c_out = fin ? 0 : end - std::max(0ll, (e1 / L) * M - width);
    if (c_in > RS_CARRY || c_out > RS_CARRY)
      return fail("%s: resampler stream %d: a carry of %lld samples exceeds the %d a slot keeps", who, i, std::max(c_in, c_out), RS_CARRY);
    if (w.c_in != c_in || w.c_out != c_out)
      return fail("%s: resampler stream %d: the step carries %lld samples in and %lld out, got %d and %d", who, i, c_in, c_out, w.c_in, w.c_out);
    *n_out_max = std::max(*n_out_max, (long long)w.n_out);
  }
  return 0;
}
extern "C" int ctts_resample_stream_step(const float* x, int64_t n_x, const ctts_rs_stream* st_dev, const ctts_rs_stream* st_host,
                                         int32_t n_streams, float* y, int64_t n_y, float* carry, int32_t n_slots, const float* taps, int32_t L,
                                         int32_t M, int32_t K, void* stream) {
  const char* who = "ctts_resample_stream_step";
  if (!st_dev || !st_host || !carry) return fail("%s: a null pointer (both descriptor tables and the carry are needed)", who);
  if (n_x < 0 || n_y < 0 || (!x && n_x) || (!y && n_y)) return fail("%s: a null pointer (x or y) with a length other than 0", who);
  if (n_streams < 1 || n_streams > 1024) return fail("%s: need 1 <= n_streams <= 1024 (got %d)", who, n_streams);
  if (n_slots < 1) return fail("%s: the state pool has no slot", who);
  if (check_rs_pair(who, taps, L, M, K)) return -1;
  std::vector<char> seen((size_t)n_slots, 0);
  long long n_out_max = 0;
  if (check_rs_streams(who, st_host, 0, n_streams, n_x, n_y, n_slots, L, M, K, seen, &n_out_max)) return -1;
  CttsDeviceGuard dg(stream);
  CK(launch_resample_stream(x, (const RsStream*)st_dev, n_streams, n_out_max, y, carry, taps, L, M, K, (hipStream_t)stream));
  return 0;
}

// ---- window decode of time-scaled streams: crop -> stream step -> 16-bit conversion, around ONE ragged decoder pass --------------------
// workspace = the window-decode workspace (n_win >= 1) | the scaled chunks, each from a multiple of 8 floats on | the path entries
extern "C" size_t ctts_codec_windows_speed_workspace_bytes(int32_t n_win, int32_t total_tokens, int64_t chunk_floats) {
  if (n_win < 0 || chunk_floats < 0 || chunk_floats >= (1ll << 31)) return 0;
  const size_t base = n_win ? ctts_codec_windows_workspace_bytes(n_win, total_tokens) : 0;
  if (n_win && base == 0) return 0;
  return base + align_up((size_t)chunk_floats * 4 + 16);
}
// the resampler stage behind the time scaler (ctts_codec_decode_windows_speed_rate); null: there is none
struct RsStage {
  const ctts_rs_stream *dev, *host;
  const int32_t *of_ts, *grp_off, *grp_rate;
  int n_grp;
  const ctts_rate* rates;
  int n_rates;
  float* carry;
  int n_slots;
};
static int decode_windows_speed_body(const char* who, ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots,
                                     int32_t hid_cap, const ctts_window* win_dev, const ctts_window* win_host, int32_t n_win,
                                     const ctts_window* cwin_dev, const ctts_window* cwin_host, const ctts_rs_window* crs_dev,
                                     const ctts_rs_window* crs_host, int32_t n_conv, const ctts_ts_stream* ts_dev,
                                     const ctts_ts_stream* ts_host, const int32_t* round_off, int32_t n_rounds, float* carry,
                                     int32_t* state, int32_t n_ts_slots, const float* ts_window, const RsStage* rs, int32_t out_type, void* out,
                                     uint8_t* keep_bits, int32_t product, float keep_thr, void* workspace, size_t ws_bytes, void* stream) {
  if (!c || !cwin_dev || !cwin_host || !crs_dev || !crs_host || !ts_dev || !ts_host || !round_off || !carry || !state || !ts_window || !out)
    return fail("%s: a null pointer", who);
  if (n_win < 0 || n_win > 1024 || (n_win && (!hid || !win_dev || !win_host))) return fail("%s: need 0 <= n_win <= 1024 and, with windows, the store and their tables", who);
  if (n_conv < 1 || n_conv > 2048) return fail("%s: need 1 <= n_conv <= 2048 (got %d)", who, n_conv);
  if (n_rounds < 1 || n_rounds > n_conv || round_off[0] != 0) return fail("%s: need 1 <= n_rounds <= n_conv, the first round at 0", who);
  for (int r = 0; r < n_rounds; ++r)
    if (round_off[r + 1] <= round_off[r]) return fail("%s: round %d is empty", who, r);
  const int n_ts = round_off[n_rounds];
  if (n_ts > n_conv) return fail("%s: %d stream descriptors for %d chunks", who, n_ts, n_conv);
  if (n_ts_slots < 1) return fail("%s: the state pool has no slot", who);
  if (check_out_format(who, out_type, product, out) || (n_win && check_store(who, hid, slot_stride, row_stride, n_slots, hid_cap))) return -1;
  std::vector<int32_t> tok;
  if (check_windows(who, win_host, n_win, n_slots, hid_cap, tok)) return -1;
  const int T = tok[n_win];
  const long long n_x = n_win ? 256 * (2 * (long long)T - n_win) : 0;
  // what chunk e of the output is: a 24 kHz crop of the packed decode (rate < 0), or the chunk of stream descriptor `rate`
  std::vector<char> used((size_t)n_ts, 0);
  long long chunk_floats = 0, n_path = 0;
  for (int e = 0; e < n_conv; ++e) {
    const ctts_rs_window& r = crs_host[e];
    if (cwin_host[e].keep && !keep_bits) return fail("%s: chunk %d asks for a keep mask but keep_bits is null", who, e);
    if (r.rate < 0) {
      if (r.in_off < 0 || r.n_in < 1 || r.in_off + r.n_in > n_x) return fail("%s: chunk %d: the crop lies outside the packed decode (%lld floats)", who, e, n_x);
      continue;
    }
    if (r.rate >= n_ts || used[r.rate]) return fail("%s: chunk %d names stream descriptor %d of %d, or one that is taken", who, e, r.rate, n_ts);
    used[r.rate] = 1;
    const ctts_ts_stream& t = ts_host[r.rate];
    const bool resampled = rs && rs->of_ts[r.rate] >= 0;       // the entry then describes the resampled chunk: checked below
    if (t.n_out < 0 || t.out_off != chunk_floats || (!resampled && (r.o_lo != 0 || r.o_hi != t.n_out || r.out_off != chunk_floats)))
      return fail("%s: chunk %d: the scaled chunks lie one behind the other, each from a multiple of 8 floats on", who, e);
    if (t.path_off != n_path) return fail("%s: chunk %d: the path entries lie one behind the other", who, e);
    chunk_floats += ((long long)t.n_out + 7) & ~7ll;
    n_path += ts_path_entries(t);
  }
  for (int q = 0; q < n_ts; ++q)
    if (!used[q]) return fail("%s: stream descriptor %d belongs to no chunk", who, q);
  const long long ts_floats = chunk_floats;                    // the scaled chunks: what the resampler stage reads
  const int n_rs = rs ? rs->grp_off[rs->n_grp] : 0;
  if (rs) {
    std::vector<char> taken((size_t)n_rs, 0);
    for (int e = 0; e < n_conv; ++e) {
      const ctts_rs_window& r = crs_host[e];
      if (r.rate < 0 || rs->of_ts[r.rate] < 0) continue;
      const int q = rs->of_ts[r.rate];
      if (q >= n_rs || taken[q]) return fail("%s: chunk %d names resampler descriptor %d of %d, or one that is taken", who, e, q, n_rs);
      taken[q] = 1;
      const ctts_ts_stream& t = ts_host[r.rate];
      const ctts_rs_stream& w = rs->host[q];
      if (w.in_off != t.out_off || w.n_in != t.n_out) return fail("%s: chunk %d: the resampler's push is not the scaled chunk", who, e);
      if (w.n_out < 0 || w.out_off != chunk_floats || w.pad != (int)(((w.n_out + 7) & ~7ll) - w.n_out) || r.o_lo != 0 || r.o_hi != w.n_out ||
          r.out_off != w.out_off)
        return fail("%s: chunk %d: the resampled chunks lie behind the scaled ones, one behind the other, each from a multiple of 8 floats on", who, e);
      chunk_floats += w.n_out + w.pad;
    }
    for (int q = 0; q < n_rs; ++q)
      if (!taken[q]) return fail("%s: resampler descriptor %d belongs to no chunk", who, q);
  }
  const long long area = chunk_floats + ((n_path + 7) & ~7ll);
  const size_t need_ws = area < (1ll << 31) ? ctts_codec_windows_speed_workspace_bytes(n_win, T, area) : 0;
  if (!workspace || need_ws == 0 || ws_bytes < need_ws) return fail("codec workspace too small");
  std::vector<char> seen((size_t)n_ts_slots, 0);
  for (int r = 0; r < n_rounds; ++r)
    if (check_ts_streams(who, ts_host, round_off[r], round_off[r + 1], n_x, ts_floats, n_path, n_ts_slots, seen)) return -1;
  std::vector<long long> rs_longest((size_t)(rs ? rs->n_grp : 0), 0);
  if (rs) {
    std::vector<char> rs_seen((size_t)rs->n_slots, 0);
    for (int g = 0; g < rs->n_grp; ++g) {
      const ctts_rate& p = rs->rates[rs->grp_rate[g]];
      if (check_rs_streams(who, rs->host, rs->grp_off[g], rs->grp_off[g + 1], ts_floats, chunk_floats, rs->n_slots, p.L, p.M, p.K, rs_seen,
                           &rs_longest[g]))
        return -1;
    }
  }
  const float* wav = nullptr;
  float* chunks = (float*)workspace;
  if (n_win) {
    WindowsWs ws = carve_windows(workspace, n_win, T);
    wav = ws.wav;
    chunks = (float*)((char*)workspace + ws.bytes);
    if (decode_windows_front(c, hid, slot_stride, row_stride, win_dev, n_win, tok, ws, workspace, stream)) return -1;
  }
  int32_t* path = (int32_t*)(chunks + chunk_floats);
  CttsDeviceGuard dg(stream);
  for (int r = 0; r < n_rounds; ++r)      // a stream with several chunks in the call takes them one launch after the other
    CK(launch_time_scale_stream(wav, (const TsStream*)ts_dev + round_off[r], round_off[r + 1] - round_off[r], chunks, path, carry, state, ts_window,
                                (hipStream_t)stream));
  if (rs)                                 // behind every round of the scaler: one launch per group (a round's descriptors at one rate)
    for (int g = 0; g < rs->n_grp; ++g) {
      const ctts_rate& p = rs->rates[rs->grp_rate[g]];
      CK(launch_resample_stream(chunks, (const RsStream*)rs->dev + rs->grp_off[g], rs->grp_off[g + 1] - rs->grp_off[g], rs_longest[g], chunks,
                                rs->carry, p.taps, p.L, p.M, p.K, (hipStream_t)stream));
    }
  CK(launch_chunks_pcm16(wav, chunks, (const CodecWindow*)cwin_dev, (const RsWindow*)crs_dev, n_conv, out_type == 0 ? 1 : 0, product, keep_thr,
                         out, keep_bits, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_codec_decode_windows_speed(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots,
                                               int32_t hid_cap, const ctts_window* win_dev, const ctts_window* win_host, int32_t n_win,
                                               const ctts_window* cwin_dev, const ctts_window* cwin_host, const ctts_rs_window* crs_dev,
                                               const ctts_rs_window* crs_host, int32_t n_conv, const ctts_ts_stream* ts_dev,
                                               const ctts_ts_stream* ts_host, const int32_t* round_off, int32_t n_rounds, float* carry,
                                               int32_t* state, int32_t n_ts_slots, const float* ts_window, int32_t out_type, void* out,
                                               uint8_t* keep_bits, int32_t product, float keep_thr, void* workspace, size_t ws_bytes, void* stream) {
  return decode_windows_speed_body("ctts_codec_decode_windows_speed", c, hid, slot_stride, row_stride, n_slots, hid_cap, win_dev, win_host, n_win,
                                   cwin_dev, cwin_host, crs_dev, crs_host, n_conv, ts_dev, ts_host, round_off, n_rounds, carry, state, n_ts_slots,
                                   ts_window, nullptr, out_type, out, keep_bits, product, keep_thr, workspace, ws_bytes, stream);
}

// ---- the same with the resampler stage: crop -> time scaler's stream step -> resampler's stream step -> 16-bit conversion --------------
extern "C" size_t ctts_codec_windows_speed_rate_workspace_bytes(int32_t n_win, int32_t total_tokens, int64_t chunk_floats) {
  return ctts_codec_windows_speed_workspace_bytes(n_win, total_tokens, chunk_floats);
}
extern "C" int ctts_codec_decode_windows_speed_rate(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots,
                                                    int32_t hid_cap, const ctts_window* win_dev, const ctts_window* win_host, int32_t n_win,
                                                    const ctts_window* cwin_dev, const ctts_window* cwin_host, const ctts_rs_window* crs_dev,
                                                    const ctts_rs_window* crs_host, int32_t n_conv, const ctts_ts_stream* ts_dev,
                                                    const ctts_ts_stream* ts_host, const int32_t* round_off, int32_t n_rounds, float* carry,
                                                    int32_t* state, int32_t n_ts_slots, const float* ts_window, const ctts_rs_stream* rs_dev,
                                                    const ctts_rs_stream* rs_host, const int32_t* rs_of_ts, const int32_t* grp_off,
                                                    const int32_t* grp_rate, int32_t n_grp, const ctts_rate* rates, int32_t n_rates,
                                                    float* rs_carry, int32_t n_rs_slots, int32_t out_type, void* out, uint8_t* keep_bits,
                                                    int32_t product, float keep_thr, void* workspace, size_t ws_bytes, void* stream) {
  const char* who = "ctts_codec_decode_windows_speed_rate";
  if (!rs_of_ts || !grp_off) return fail("%s: a null pointer (the chunks' resampler descriptors and the group offsets are needed)", who);
  if (n_grp < 0 || n_grp > 2048 || grp_off[0] != 0) return fail("%s: need 0 <= n_grp <= 2048, the first group at 0", who);
  if (n_grp && (!rs_dev || !rs_host || !grp_rate || !rates || !rs_carry)) return fail("%s: a null pointer (the resampler stage's tables and carry)", who);
  if (n_grp && n_rs_slots < 1) return fail("%s: the resampler's state pool has no slot", who);
  if (n_rates < 0 || n_rates > 2048) return fail("%s: need 0 <= n_rates <= 2048", who);
  for (int r = 0; r < n_rates; ++r)
    if (check_rs_pair(who, rates[r].taps, rates[r].L, rates[r].M, rates[r].K)) return -1;
  for (int g = 0; g < n_grp; ++g) {
    if (grp_off[g + 1] <= grp_off[g] || grp_off[g + 1] > 2048) return fail("%s: resampler group %d is empty, or the table holds more than 2048", who, g);
    if (grp_rate[g] < 0 || grp_rate[g] >= n_rates) return fail("%s: resampler group %d names rate %d of %d", who, g, grp_rate[g], n_rates);
  }
  const RsStage rs{rs_dev, rs_host, rs_of_ts, grp_off, grp_rate, n_grp, rates, n_rates, rs_carry, n_rs_slots};
  return decode_windows_speed_body(who, c, hid, slot_stride, row_stride, n_slots, hid_cap, win_dev, win_host, n_win, cwin_dev, cwin_host, crs_dev,
                                   crs_host, n_conv, ts_dev, ts_host, round_off, n_rounds, carry, state, n_ts_slots, ts_window, &rs, out_type, out,
                                   keep_bits, product, keep_thr, workspace, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// single-kernel entry points
// ------------------------------------------------------------------------------------------------
extern "C" int ctts_k_gemm(int32_t tiled, const float* A, const void* W, float* C, int32_t M, int32_t N, int32_t K, int32_t lda,
                           int32_t ldc, int32_t wt, int32_t epi, const float* norm_w, float eps, const float* res, int32_t ldr,
                           const float* bias, const float* gamma, int32_t taps, int32_t cin, int32_t frames, int32_t pad, int32_t dil,
                           void* stream) {
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.W = W; a.C = C; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.wt = wt; a.epi = epi; a.norm_w = norm_w; a.eps = eps;
  a.res = res; a.ldr = ldr; a.bias = bias; a.gamma = gamma; a.taps = taps > 0 ? taps : 1; a.cin = cin; a.frames = frames; a.pad = pad;
  a.dil = dil;
  { const char* e = getenv("CTTS_X3_DBG_PTR"); if (e) a.dbg = (long long*)strtoull(e, nullptr, 0); }   // probe builds only
  CK(tiled == 2 ? launch_gemm_tiled_bf16x3(a, (hipStream_t)stream) : tiled ? launch_gemm_tiled(a, (hipStream_t)stream) : launch_gemm_skinny(a, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_x3p(const uint16_t* Ap, const uint16_t* Wp, int32_t M, int32_t N, int32_t K, int32_t epi, const float* bias,
                               const float* gamma, const float* res, float* C, uint16_t* Cp, void* stream) {
  X3pArgs g;
  memset(&g, 0, sizeof(g));
  g.Ap = Ap; g.Wp = Wp; g.M = M; g.N = N; g.K = K; g.epi = epi; g.bias = bias; g.gamma = gamma; g.res = res; g.ldr = N; g.C = C; g.ldc = N; g.Cp = Cp;
  { const char* e = getenv("CTTS_X3_DBG_PTR"); if (e) g.dbg = (long long*)strtoull(e, nullptr, 0); }   // probe variant only
  CK(launch_gemm_x3p(g, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_h1p(const uint16_t* Ap, const uint16_t* Wp, int32_t M, int32_t N, int32_t K, int32_t epi, const float* bias,
                               const float* gamma, const float* res, float* C, uint16_t* Cp, void* stream) {
  X3pArgs g;
  memset(&g, 0, sizeof(g));
  g.Ap = Ap; g.Wp = Wp; g.M = M; g.N = N; g.K = K; g.epi = epi; g.bias = bias; g.gamma = gamma; g.res = res; g.ldr = N; g.C = C; g.ldc = N; g.Cp = Cp;
  { const char* e = getenv("CTTS_X3_DBG_PTR"); if (e) g.dbg = (long long*)strtoull(e, nullptr, 0); }   // probe variant only (CTTS_H1P_PROBE=1)
  CK(launch_gemm_h1p(g, (hipStream_t)stream));
  return 0;
}
// ------------------------------------------------------------------------------------------------
// A HIP stream confined to a subset of the CUs (hipExtStreamCreateWithCUMask): the acoustic decoder of batch i on a side stream of a few CUs
// while batch i + 1 is generated on the rest (CodecEngine.decode_to_wavs_async, CTTS_CODEC_CUS).  CUs first, first + stride, ... (n of them).
// ------------------------------------------------------------------------------------------------
extern "C" int ctts_stream_create_cu_mask(int32_t first_cu, int32_t n_cus, int32_t stride, int32_t complement, void** stream) {
  if (!stream || n_cus <= 0 || first_cu < 0 || stride <= 0) return fail("ctts_stream_create_cu_mask: bad arguments");
  int dev = 0, ncu = 0;
  CK(hipGetDevice(&dev));
  CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
  int set = 0;
  for (int i = 0; i < n_cus; ++i) {
    const int cu = first_cu + i * stride;
    if (cu >= ncu) break;
    mask[cu >> 5] |= 1u << (cu & 31);
    ++set;
  }
  if (complement) {   // every CU of the device EXCEPT those: the stream of the work the confined stream must not disturb
    for (int cu = 0; cu < ncu; ++cu) mask[cu >> 5] ^= 1u << (cu & 31);
    set = ncu - set;
  }
  if (set <= 0) return fail("ctts_stream_create_cu_mask: no CU selected");
  hipStream_t st = nullptr;
  CK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
  *stream = (void*)st;
  return 0;
}
extern "C" int ctts_stream_destroy(void* stream) {
  if (stream) CK(hipStreamDestroy((hipStream_t)stream));
  return 0;
}

extern "C" int ctts_k_mlp_fused(const uint16_t* Ap, const uint16_t* W1p, const uint16_t* W2p, int32_t M, int32_t inter, const float* b1,
                                const float* b2, const float* gamma, float* C, int32_t planes, void* stream) {
  if (planes != 1) return fail("ctts_k_mlp_fused: planes must be 1 (fp16 plane)");
  MlpArgs m;
  memset(&m, 0, sizeof(m));
  m.Ap = Ap; m.W1p = W1p; m.W2p = W2p; m.M = M; m.inter = inter; m.b1 = b1; m.b2 = b2; m.gamma = gamma; m.C = C;
  { const char* e = getenv("CTTS_X3_DBG_PTR"); if (e) m.dbg = (long long*)strtoull(e, nullptr, 0); }   // probe only
  CK(launch_mlp_fused_h1p(m, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_fast(const uint16_t* A, int32_t lda, const uint16_t* W, int32_t M, int32_t N, int32_t K, const float* ssq_in,
                                float eps, int32_t epi, float* C32, int32_t ldc, uint16_t* Cb, int32_t ldcb, float* ssq_out, void* stream) {
  FastGemmArgs f;
  memset(&f, 0, sizeof(f));
  f.A = A; f.lda = lda; f.W = W; f.M = M; f.N = N; f.K = K; f.ssq_in = ssq_in; f.eps = eps; f.epi = epi; f.C32 = C32; f.ldc = ldc;
  f.Cb = Cb; f.ldcb = ldcb; f.ssq_out = ssq_out;
  { const char* e = getenv("CTTS_GEMM_DBG_PTR"); if (e) f.dbg = (long long*)strtoull(e, nullptr, 0); }
  CK(launch_gemm_fast(f, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_qkv_rope(const uint16_t* A, const uint16_t* W, int32_t M, const float* ssq_in, float eps, float* qkv, uint16_t* kcache,
                               uint16_t* vcache, int32_t cmax, const float* cos_tab, const float* sin_tab, int32_t q_per_b,
                               const int32_t* len, const int32_t* kv_start, int32_t force_mb, void* stream) {
  FastGemmArgs f;
  memset(&f, 0, sizeof(f));
  f.A = A; f.lda = HID; f.W = W; f.M = M; f.N = 3 * HID; f.K = HID; f.ssq_in = ssq_in; f.eps = eps; f.epi = FEPI_QKV_ROPE; f.C32 = qkv;
  f.ldc = 3 * HID; f.q_per_b = q_per_b; f.len = len; f.kv_start = kv_start; f.cos_t = cos_tab; f.sin_t = sin_tab; f.kc = kcache;
  f.vc = vcache; f.cmax = cmax; f.force_mb = force_mb;
  CK(launch_gemm_fast(f, (hipStream_t)stream));
  return 0;
}
// the same with the prompt chunk's first slot and the slot-pool row_map that run_step passes (tests)
extern "C" int ctts_k_qkv_rope_ex(const uint16_t* A, const uint16_t* W, int32_t M, const float* ssq_in, float eps, float* qkv, uint16_t* kcache,
                                  uint16_t* vcache, int32_t cmax, const float* cos_tab, const float* sin_tab, int32_t q_per_b,
                                  const int32_t* len, const int32_t* kv_start, int32_t slot0, const int32_t* row_map, int32_t force_mb,
                                  void* stream) {
  const char* who = "ctts_k_qkv_rope_ex";
  if (!A || !W || !ssq_in || !qkv || !kcache || !vcache || !cos_tab || !sin_tab || !kv_start) return fail("%s: null pointer", who);
  if (q_per_b < 1 || M <= 0 || (q_per_b == 1 && !len)) return fail("%s: bad q_per_b / M (q_per_b == 1 is a decode launch and needs len)", who);
  if (q_per_b > 1 && (M % q_per_b != 0 || slot0 < 0 || slot0 + q_per_b > cmax))
    return fail("%s: M must be a multiple of q_per_b and slots [slot0, slot0 + q_per_b) must lie inside the cache rows", who);
  FastGemmArgs f;
  memset(&f, 0, sizeof(f));
  f.A = A; f.lda = HID; f.W = W; f.M = M; f.N = 3 * HID; f.K = HID; f.ssq_in = ssq_in; f.eps = eps; f.epi = FEPI_QKV_ROPE; f.C32 = qkv;
  f.ldc = 3 * HID; f.q_per_b = q_per_b; f.len = len; f.kv_start = kv_start; f.cos_t = cos_tab; f.sin_t = sin_tab; f.kc = kcache;
  f.vc = vcache; f.cmax = cmax; f.force_mb = force_mb; f.slot0 = slot0; f.row_map = row_map;
  CK(launch_gemm_fast(f, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_dec(const uint16_t* Ap, const uint16_t* Wp, int32_t M, int32_t N, int32_t K, const int32_t* n_active,
                               const float* ssq_in, float eps, int32_t epi, float* C32, int32_t ldc, uint16_t* Cp, int32_t kch_out,
                               float* ssq_out, int32_t force_mb, void* stream) {
  if (epi == FEPI_QKV_ROPE) return fail("ctts_k_gemm_dec: the fused QKV epilogue is reached through the decode step only");
  DecGemmArgs d;
  memset(&d, 0, sizeof(d));
  d.Ap = Ap; d.Wp = Wp; d.M = M; d.N = N; d.K = K; d.n_active = n_active; d.ssq_in = ssq_in; d.eps = eps; d.epi = epi; d.C32 = C32;
  d.ldc = ldc; d.Cp = Cp; d.kch_out = kch_out; d.ssq_out = ssq_out; d.force_mb = force_mb;
  { const char* e = getenv("CTTS_GEMM_DBG_PTR"); if (e) d.dbg = (long long*)strtoull(e, nullptr, 0); }   // probes only
  CK(launch_gemm_dec(d, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_dec32(const float* Ap, const float* Wp, int32_t M, int32_t N, int32_t K, const int32_t* n_active, const float* X,
                                 int32_t ldx, const float* norm_w, float eps, int32_t epi, float* C, int32_t ldc, const float* res, int32_t ldr,
                                 float* Cp, int32_t kch_out, int32_t force_mb, int32_t n_cols, void* stream) {
  Dec32Args d;
  memset(&d, 0, sizeof(d));
  d.n_cols = n_cols;
  d.Ap = Ap; d.Wp = Wp; d.M = M; d.N = N; d.K = K; d.n_active = n_active; d.X = X; d.ldx = ldx; d.norm_w = norm_w; d.eps = eps; d.epi = epi;
  d.C = C; d.ldc = ldc; d.res = res; d.ldr = ldr; d.Cp = Cp; d.kch_out = kch_out; d.force_mb = force_mb;
  CK(launch_gemm_dec32(d, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_dec32x(const uint16_t* Ap, int64_t a_plane, const uint16_t* Wp, int64_t w_plane, int32_t M, int32_t N, int32_t K,
                                  const int32_t* n_active, const float* X, int32_t ldx, float eps, int32_t epi, float* C, int32_t ldc,
                                  const float* res, int32_t ldr, uint16_t* Cp, int64_t c_plane, int32_t kch_out, float* Cp32, int32_t force_mb,
                                  const float* ssq_in, float* ssq_out, void* stream) {
  Dec32xArgs d;
  memset(&d, 0, sizeof(d));
  d.ssq_in = ssq_in; d.ssq_out = ssq_out;
  d.Ap = Ap; d.a_plane = (size_t)a_plane; d.Wp = Wp; d.w_plane = (size_t)w_plane; d.M = M; d.N = N; d.K = K; d.n_active = n_active;
  d.rms = X != nullptr || ssq_in != nullptr; d.X = X; d.ldx = ldx; d.eps = eps; d.epi = epi; d.C = C; d.ldc = ldc; d.res = res; d.ldr = ldr;
  d.Cp = Cp; d.c_plane = (size_t)c_plane; d.kch_out = kch_out; d.Cp32 = Cp32; d.kch32_out = N / 16; d.force_mb = force_mb;
  CK(launch_gemm_dec32x(d, (hipStream_t)stream));
  return 0;
}
extern "C" const char* ctts_k_dec32_last_variant(void) { return dec32_last_variant(); }
extern "C" int ctts_k_rows_prep(const float* x32, uint16_t* xb, float* ssq, int32_t M, void* stream) {
  CK(launch_rows_prep(x32, xb, ssq, M, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_rope_append(float* qkv, void* kcache, void* vcache, int32_t kv_dtype, int32_t cmax, const float* cos_tab,
                                  const float* sin_tab, int32_t q_per_b, const int32_t* len, const int32_t* kv_start, int32_t M,
                                  void* stream) {
  GptRowMap rm{q_per_b, len, kv_start, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
  CK(launch_rope_append(qkv, kcache, vcache, kv_dtype, cmax, cos_tab, sin_tab, rm, M, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_attention(const float* qkv, const void* kcache, const void* vcache, int32_t kv_dtype, int32_t cmax, float* out,
                                int32_t q_per_b, const int32_t* len, const int32_t* kv_start, int32_t M, void* stream) {
  GptRowMap rm{q_per_b, len, kv_start, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
  CK(launch_attention(qkv, kcache, vcache, kv_dtype, cmax, out, 0, rm, M, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_attention_prefill(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, float* out, int32_t q_per_b,
                                        int32_t slot0, const int32_t* kv_start, int32_t M, void* stream) {
  GptRowMap rm{q_per_b, nullptr, kv_start, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, slot0, 0};
  CK(launch_attention(qkv, kcache, vcache, WT_BF16, cmax, out, 0, rm, M, (hipStream_t)stream));
  return 0;
}
// the prompt pass's attention as run_step launches it (tests): the shipped bf16-output instantiations and the slot-pool row_map
extern "C" int ctts_k_attention_prefill_ex(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, void* out, int32_t out_bf16,
                                           int32_t q_per_b, int32_t slot0, const int32_t* kv_start, const int32_t* row_map, int32_t M,
                                           void* stream) {
  const char* who = "ctts_k_attention_prefill_ex";
  if (!qkv || !kcache || !vcache || !out || !kv_start) return fail("%s: null pointer", who);
  if (out_bf16 != 0 && out_bf16 != 1) return fail("%s: out_bf16 is 0 (f32) or 1 (bf16)", who);
  // q_per_b == 1 is the decode convention of GptRowMap (slot = len[b] - 1): not a prompt pass, and there is no `len` here
  if (q_per_b < 2 || M <= 0 || M % q_per_b != 0) return fail("%s: M must be a positive multiple of q_per_b >= 2", who);
  if (slot0 < 0 || slot0 + q_per_b > cmax) return fail("%s: slots [slot0, slot0 + q_per_b) must lie inside the cache rows", who);
  GptRowMap rm{q_per_b, nullptr, kv_start, row_map, nullptr, nullptr, nullptr, nullptr, nullptr, 0, slot0, 0};
  CK(launch_attention(qkv, kcache, vcache, WT_BF16, cmax, out, out_bf16, rm, M, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_attention_dec(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, uint16_t* out_packed,
                                    const int32_t* desc, const int32_t* n_active, int32_t M, float* part, int32_t* cnt, int32_t n_cu,
                                    void* stream) {
  if (n_cu < 0 || n_cu > ATT_CUS_MAX) return fail("ctts_k_attention_dec: bad n_cu");
  GptRowMap rm{1, nullptr, nullptr, nullptr, n_active, nullptr, reinterpret_cast<const RowDesc*>(desc), part, cnt, n_cu, 0, 0};
  CK(launch_attention(qkv, kcache, vcache, WT_BF16, cmax, out_packed, 2, rm, M, (hipStream_t)stream));
  return 0;
}
// decode attention of either mode on fragment-packed output, straight to launch_attention (kv_dtype CTTS_BF16: bf16 cache, packed bf16 output;
// CTTS_F32: f32 cache, packed f32 output); `covers_all`: descriptors are valid for all M rows (absent rows carry b = -1) and n_active is not read
extern "C" int ctts_k_attention_dec2(const float* qkv, const void* kcache, const void* vcache, int32_t kv_dtype, int32_t cmax, void* out_packed,
                                     const int32_t* desc, const int32_t* n_active, int32_t covers_all, int32_t M, void* stream) {
  if (!desc || M <= 0 || kv_dtype < 0 || kv_dtype > 2) return fail("ctts_k_attention_dec2: bad arguments");
  GptRowMap rm{1, nullptr, nullptr, nullptr, n_active, nullptr, reinterpret_cast<const RowDesc*>(desc), nullptr, nullptr, 0, 0, covers_all};
  if (kv_dtype == 2) rm.x3_plane = ((size_t)M + 15) / 16 * 16 * HID;   // f32 cache, output as hi | lo bf16 planes (the split-bf16 parity mode)
  CK(launch_attention(qkv, kcache, vcache, kv_dtype == CTTS_BF16 ? WT_BF16 : WT_F32, cmax, out_packed, kv_dtype == CTTS_BF16 ? 2 : kv_dtype == 2 ? 4 : 3, rm, M,
                      (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_attention_cfg(int32_t persist, int32_t workgroups, int32_t ring) {
  if (ring > 0 && ring != 2 && ring != 3 && ring != 4) return fail("ctts_k_attention_cfg: ring depth must be 2, 3 or 4");
  attention_persist_override(persist, workgroups, ring);
  return 0;
}
extern "C" int ctts_k_attention_heads_per_wg(int32_t hpw) {
  if (hpw != 1 && hpw != 2 && hpw != 3 && hpw != 4) return fail("ctts_k_attention_heads_per_wg: 1, 2, 3 or 4");
  attention_hpw_override(hpw);
  return 0;
}
extern "C" int ctts_k_attention_oproj(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, const uint16_t* wo_hd,
                                      const int32_t* desc, const int32_t* n_active, int32_t M, float* part, int32_t* cnt, float* x32,
                                      uint16_t* xp, float* ssq, void* stream) {
  if (!wo_hd || !desc || !part || !cnt || !x32 || !xp || !ssq || M <= 0) return fail("ctts_k_attention_oproj: bad arguments");
  GptRowMap rm{1, nullptr, nullptr, nullptr, n_active, nullptr, reinterpret_cast<const RowDesc*>(desc), nullptr, nullptr, 0, 0, 0};
  rm.wo_h = wo_hd; rm.op_part = part; rm.op_part_bytes = (int)((size_t)((M + 15) / 16 * 16) * NHEAD * HID * sizeof(float)); rm.op_cnt = cnt;
  rm.x32 = x32; rm.xp = xp; rm.ssq = ssq;
  CK(launch_attention_oproj(qkv, kcache, vcache, cmax, rm, M, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_embed_codes(const float* emb_code, const int64_t* ids_buf, int32_t tcap, const int32_t* len, float* x, int32_t B,
                                  void* stream) {
  CK(launch_embed_codes(emb_code, ids_buf, tcap, len, x, nullptr, nullptr, B, nullptr, nullptr, (hipStream_t)stream));
  return 0;
}
// ---- the row-descriptor contract, kernel by kernel (tests/test_gpu_step_front.py, tests/test_gpu_parity_qkv.py) ----------------------
// the step's first kernel with a caller-filled StepPrep: embed_codes_k, or embed_text_k when n_text > 0
extern "C" int ctts_k_step_prep(const float* emb, int32_t n_text, const int64_t* ids_buf, int32_t tcap, const int32_t* len, float* x,
                                uint16_t* xb, float* ssq, int32_t B, const int32_t* row_map, const int32_t* n_active, int32_t* desc,
                                const int32_t* kv_start, const uint8_t* finish, int32_t xb_packed, float* xp32, int64_t xb_lo_plane,
                                int32_t* row_map_out, int32_t* n_active_out, const int32_t* order, float* rope_cs, const float* cos_tab,
                                const float* sin_tab, int32_t* zero_p, int32_t zero_n, int32_t zero_stride, void* stream) {
  const char* who = "ctts_k_step_prep";
  if (!emb || !ids_buf || !len || !x || B <= 0 || tcap <= 0 || n_text < 0) return fail("%s: bad arguments", who);
  if ((desc || rope_cs) && !kv_start) return fail("%s: descriptors and RoPE rows need kv_start", who);
  if (rope_cs && (!cos_tab || !sin_tab)) return fail("%s: rope_cs needs the cos / sin tables", who);
  if (row_map_out && (!finish || !n_active_out)) return fail("%s: device-side compaction needs finish and n_active_out", who);
  if (xb_lo_plane < 0 || (xb_lo_plane & 7) || (xb_lo_plane && (!xb || !xb_packed))) return fail("%s: the lo plane needs a packed xb, a multiple of 8 elements behind it", who);
  if (zero_p && (zero_n < 0 || zero_stride < 1)) return fail("%s: bad zero_n / zero_stride", who);
  StepPrep sp{reinterpret_cast<RowDesc*>(desc), kv_start, finish, xb_packed ? 1 : 0, xp32, row_map_out, n_active_out, order, rope_cs, cos_tab, sin_tab,
              zero_p, zero_n, zero_stride, (size_t)xb_lo_plane};
  if (n_text > 0) CK(launch_embed_text(emb, n_text, ids_buf, tcap, len, x, xb, ssq, B, row_map, n_active, (hipStream_t)stream, &sp));
  else CK(launch_embed_codes(emb, ids_buf, tcap, len, x, xb, ssq, B, row_map, n_active, (hipStream_t)stream, &sp));
  return 0;
}
extern "C" int ctts_k_prefill_prep32(const float* x, float* xp32, int32_t* desc, int32_t q_per_b, int32_t slot0, const int32_t* kv_start,
                                     const int32_t* row_map, int32_t M, void* stream) {
  if (!x || !xp32 || !desc || !kv_start || q_per_b <= 0 || slot0 < 0 || M <= 0) return fail("ctts_k_prefill_prep32: bad arguments");
  CK(launch_prefill_prep32(x, xp32, reinterpret_cast<RowDesc*>(desc), q_per_b, slot0, kv_start, row_map, M, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_prefill_compact(const float* emb, float* x, int32_t* desc, int32_t* last_row, int32_t B, int32_t T, const int32_t* kv_start,
                                      void* stream) {
  if (!emb || !x || !desc || !last_row || !kv_start || B <= 0 || T <= 0) return fail("ctts_k_prefill_compact: bad arguments");
  CK(launch_prefill_compact(emb, x, reinterpret_cast<RowDesc*>(desc), last_row, B, T, kv_start, (hipStream_t)stream));
  return 0;
}
// ---- ... and its readers at the end of the step (tests/test_gpu_step_back.py) --------------------------------------------------------
// final_norm_k with every argument of launch_final_norm
extern "C" int ctts_k_final_norm_rows(const float* x, int32_t q_per_b, const float* w, float eps, float* hfin, float* hiddens, int32_t max_new,
                                      const int32_t* len, int32_t T, int32_t B, const int32_t* row_map, const int32_t* n_active,
                                      const int32_t* prompt_len, float* hfin_packed, const int32_t* last_row, void* stream) {
  const char* who = "ctts_k_final_norm_rows";
  if (!x || !w || !hfin || !len || B <= 0 || q_per_b <= 0 || T < 0) return fail("%s: bad arguments", who);
  if (hiddens && max_new <= 0) return fail("%s: hiddens needs max_new > 0", who);
  if (n_active && q_per_b != 1) return fail("%s: n_active belongs to the decode layout (q_per_b = 1)", who);
  if (last_row && n_active) return fail("%s: last_row belongs to the prompt pass, n_active to the decode step", who);
  CK(launch_final_norm(x, q_per_b, w, eps, hfin, hiddens, max_new, len, T, B, row_map, n_active, prompt_len, (hipStream_t)stream, hfin_packed,
                       last_row));
  return 0;
}
// the decode step's one-launch final RMSNorm + hidden capture + heads (decode32.hip gemm_dec32_fnorm16_k): launch_gemm_dec32 with fnorm = 1,
// K = 768, EPI_STORE
extern "C" int ctts_k_fnorm_heads(const float* Ap, const float* Wp, int32_t M, int32_t N, int32_t n_cols, const int32_t* n_active,
                                  const float* norm_w, float eps, float* C, int32_t ldc, const int32_t* desc, float* hid, int32_t hid_cap,
                                  int32_t T, const int32_t* prompt_len, void* stream) {
  const char* who = "ctts_k_fnorm_heads";
  if (!Ap || !Wp || !norm_w || !C || M <= 0) return fail("%s: bad arguments", who);
  if (N <= 0 || (N & 15) || n_cols <= 0 || n_cols > N || ldc < n_cols) return fail("%s: N is a multiple of 16, 0 < n_cols <= N, ldc >= n_cols", who);
  if (hid && (!desc || hid_cap <= 0)) return fail("%s: the hidden capture needs desc and hid_cap > 0", who);
  if (prompt_len && !hid) return fail("%s: prompt_len is read by the hidden capture only", who);
  Dec32Args d;
  memset(&d, 0, sizeof(d));
  d.Ap = Ap; d.Wp = Wp; d.M = M; d.N = N; d.K = HID; d.n_active = n_active; d.epi = EPI_STORE; d.C = C; d.ldc = ldc; d.n_cols = n_cols;
  d.fnorm = 1; d.norm_w = norm_w; d.eps = eps; d.desc = reinterpret_cast<const RowDesc*>(desc); d.hid = hid; d.hid_cap = hid_cap; d.T = T;
  d.prompt_len = prompt_len;
  CK(launch_gemm_dec32(d, (hipStream_t)stream));
  return 0;
}
// the sampler on compact rows: launch_sample (n_text > 0: launch_sample_text) over a grid of `rows` logits rows, the state as in
// ctts_k_sample, the rows from desc or from row_map + n_active; x != NULL: with the next step's first kernel folded in (EmbedNext) -- its
// StepPrep as ctts_k_step_prep takes it, host compaction only
extern "C" int ctts_k_sample_rows(const ctts_gen_state* s, const float* logits, int32_t n_text, int32_t rows, const int32_t* row_map,
                                  const int32_t* n_active, const int32_t* desc, const float* emb_code, float* x, uint16_t* xb, float* ssq,
                                  int32_t* desc_out, const int32_t* kv_start, int32_t xb_packed, float* xp32, int64_t xb_lo_plane,
                                  float* rope_cs, const float* cos_tab, const float* sin_tab, void* stream) {
  const char* who = "ctts_k_sample_rows";
  if (!s || !logits || rows <= 0 || n_text < 0 || n_text > NTEXT_MAX) return fail("%s: bad arguments", who);
  if (rows > s->B) return fail("%s: more rows (%d) than utterance slots (%d)", who, rows, s->B);
  if (!s->ids_buf || !s->len || !s->finish || !s->end_idx) return fail("%s: ids_buf, len, finish and end_idx are needed", who);
  if (!s->rng_device && (s->nq <= 0 || !s->q)) return fail("%s: q draws missing", who);
  if (n_text > 0 && desc) return fail("%s: the text sampler reads no descriptors", who);
  if (!x && (emb_code || xb || ssq || desc_out || xp32 || rope_cs)) return fail("%s: outputs of the fold without x", who);
  SampleArgs a = make_sample_args(s, logits);
  a.B = rows; a.row_map = row_map; a.n_active = n_active; a.desc = reinterpret_cast<const RowDesc*>(desc);
  if (x) {
    if (n_text > 0) return fail("%s: the text sampler has no fold", who);
    if (!emb_code) return fail("%s: the fold needs emb_code", who);
    if (!desc || !desc_out) return fail("%s: the fold needs descriptors in and out", who);
    if (!kv_start) return fail("%s: the fold needs kv_start", who);
    if (rope_cs && (!cos_tab || !sin_tab)) return fail("%s: rope_cs needs the cos / sin tables", who);
    if (xb_lo_plane < 0 || (xb_lo_plane & 7) || (xb_lo_plane && (!xb || !xb_packed))) return fail("%s: the lo plane needs a packed xb, a multiple of 8 elements behind it", who);
    a.next.emb_code = emb_code; a.next.x = x; a.next.xb = xb; a.next.ssq = ssq;
    a.next.sp = StepPrep{reinterpret_cast<RowDesc*>(desc_out), kv_start, nullptr, xb_packed ? 1 : 0, xp32, nullptr, nullptr, nullptr, rope_cs, cos_tab, sin_tab,
                         nullptr, 0, 1, (size_t)xb_lo_plane};
  }
  if (n_text > 0) CK(launch_sample_text(a, n_text, (hipStream_t)stream));
  else CK(launch_sample(a, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_pre32(const float* Ap, const float* Wp, int32_t M, int32_t N, int32_t K, const float* X, int32_t ldx, const float* norm_w,
                                 float eps, float* rstd, int32_t epi, float* C, int32_t ldc, const float* res, int32_t ldr, float* Cp,
                                 int32_t kch_out, const int32_t* desc, const float* cos_tab, const float* sin_tab, float* kcache, float* vcache,
                                 int32_t cmax, void* stream) {
  const char* who = "ctts_k_gemm_pre32";
  if (!Ap || !Wp) return fail("%s: bad arguments", who);
  if (norm_w && (!X || !rstd || K != HID)) return fail("%s: the RMSNorm prologue needs X, rstd and K = 768 (launch_rows_rstd32)", who);
  if (epi == D32_EPI_QKV_ROPE && (!C || !cos_tab || !sin_tab || cmax <= 0)) return fail("%s: the QKV epilogue needs C, the tables and cmax", who);
  Dec32Args d;
  memset(&d, 0, sizeof(d));
  d.Ap = Ap; d.Wp = Wp; d.M = M; d.N = N; d.K = K; d.X = X; d.ldx = ldx; d.norm_w = norm_w; d.eps = eps; d.epi = epi; d.C = C; d.ldc = ldc;
  d.res = res; d.ldr = ldr; d.Cp = Cp; d.kch_out = kch_out; d.desc = reinterpret_cast<const RowDesc*>(desc); d.cos_t = cos_tab; d.sin_t = sin_tab;
  d.kc = kcache; d.vc = vcache; d.cmax = cmax;
  if (norm_w) CK(launch_rows_rstd32(X, ldx, M, eps, rstd, (hipStream_t)stream));
  CK(launch_gemm_pre32(d, norm_w ? rstd : nullptr, (hipStream_t)stream));
  return 0;
}
// the D32_EPI_QKV_ROPE launch of the decode step, given descriptors: x3 = 0: launch_gemm_dec32 (Ap / Wp packed f32, X + norm_w the RMSNorm
// prologue); x3 = 1: launch_gemm_dec32x (Ap / Wp hi planes, the lo planes a_plane / w_plane elements behind, gain folded into W, 1 / rms
// from ssq_in or else from X; rope_cs optional)
extern "C" int ctts_k_qkv_rope32(int32_t x3, const void* Ap, int64_t a_plane, const void* Wp, int64_t w_plane, int32_t M, const int32_t* n_active,
                                 const float* X, int32_t ldx, const float* norm_w, const float* ssq_in, float eps, float* qkv,
                                 const int32_t* desc, const float* rope_cs, const float* cos_tab, const float* sin_tab, float* kcache,
                                 float* vcache, int32_t cmax, int32_t force_mb, void* stream) {
  const char* who = "ctts_k_qkv_rope32";
  if (!Ap || !Wp || !qkv || !desc || !kcache || !vcache || M <= 0 || cmax <= 0) return fail("%s: bad arguments", who);
  if ((x3 == 0 || !rope_cs) && (!cos_tab || !sin_tab)) return fail("%s: needs the cos / sin tables", who);
  if (x3) {
    if (a_plane <= 0 || w_plane <= 0 || (!X && !ssq_in)) return fail("%s: the split launch needs both plane strides and X or ssq_in", who);
    Dec32xArgs d;
    memset(&d, 0, sizeof(d));
    d.Ap = (const uint16_t*)Ap; d.a_plane = (size_t)a_plane; d.Wp = (const uint16_t*)Wp; d.w_plane = (size_t)w_plane; d.M = M; d.N = 3 * HID; d.K = HID;
    d.n_active = n_active; d.rms = 1; d.X = X; d.ldx = ldx; d.eps = eps; d.ssq_in = ssq_in; d.rope_cs = rope_cs; d.epi = D32_EPI_QKV_ROPE;
    d.C = qkv; d.ldc = 3 * HID; d.desc = reinterpret_cast<const RowDesc*>(desc); d.cos_t = cos_tab; d.sin_t = sin_tab; d.kc = kcache; d.vc = vcache;
    d.cmax = cmax; d.force_mb = force_mb;
    CK(launch_gemm_dec32x(d, (hipStream_t)stream));
    return 0;
  }
  if (!X || !norm_w || rope_cs) return fail("%s: the f32 launch needs X and norm_w and reads no rope_cs", who);
  Dec32Args d;
  memset(&d, 0, sizeof(d));
  d.Ap = (const float*)Ap; d.Wp = (const float*)Wp; d.M = M; d.N = 3 * HID; d.K = HID; d.n_active = n_active; d.X = X; d.ldx = ldx; d.norm_w = norm_w;
  d.eps = eps; d.epi = D32_EPI_QKV_ROPE; d.C = qkv; d.ldc = 3 * HID; d.desc = reinterpret_cast<const RowDesc*>(desc); d.cos_t = cos_tab;
  d.sin_t = sin_tab; d.kc = kcache; d.vc = vcache; d.cmax = cmax; d.force_mb = force_mb;
  CK(launch_gemm_dec32(d, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_final_norm(const float* x, int32_t q_per_b, const float* w, float eps, float* hfin, float* hiddens,
                                 int32_t max_new, const int32_t* len, int32_t T, int32_t B, void* stream) {
  CK(launch_final_norm(x, q_per_b, w, eps, hfin, hiddens, max_new, len, T, B, nullptr, nullptr, nullptr, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gemm_pre_x3(const float* A, int32_t lda, const float* W, float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi,
                                  const float* norm_w, const float* rstd, const float* res, int32_t ldr, void* stream) {
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.taps = 1; a.A = A; a.lda = lda; a.W = W; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.wt = WT_F32; a.epi = epi;
  a.norm_w = norm_w; a.res = res; a.ldr = ldr;
  CK(launch_gemm_pre_x3(a, rstd, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_sample(const ctts_gen_state* s, const float* logits, void* stream) {
  if (!s || !logits) return fail("ctts_k_sample: bad arguments");
  CK(launch_sample(make_sample_args(s, logits), (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_sample_text(const ctts_gen_state* s, const float* logits, int32_t n_text, void* stream) {
  if (!s || !logits || n_text <= 0 || n_text > NTEXT_MAX) return fail("ctts_k_sample_text: bad arguments");
  CK(launch_sample_text(make_sample_args(s, logits), n_text, (hipStream_t)stream));
  return 0;
}
// what CttsDeviceGuard (kernels.hpp) does for `stream` on the calling thread: the device current before, the device that owns the stream,
// the device current INSIDE the guard, and whether it had to switch (tests: the guard's path runs on a 1-GPU box too)
extern "C" int ctts_k_device_guard_probe(void* stream, int32_t* before, int32_t* stream_dev, int32_t* inside, int32_t* switched) {
  if (!before || !stream_dev || !inside || !switched) return fail("ctts_k_device_guard_probe: null argument");
  int b = -1, in = -1;
  CK(hipGetDevice(&b));
  *stream_dev = -1;
  if (stream != nullptr) { hipDevice_t d; CK(hipStreamGetDevice((hipStream_t)stream, &d)); *stream_dev = (int32_t)d; }
  {
    CttsDeviceGuard dg(stream);
    CK(hipGetDevice(&in));
    *switched = dg.switched ? 1 : 0;
  }
  int after = -1;
  CK(hipGetDevice(&after));
  if (after != b) return fail("CttsDeviceGuard did not restore the current device (%d -> %d)", b, after);
  *before = b; *inside = in;
  return 0;
}
extern "C" int ctts_float_to_int16(const float* wav, int16_t* pcm, uint8_t* keep_bits, int32_t rows, int64_t n, int64_t ld, int32_t per_row,
                                   int32_t product, float keep_thr, uint32_t* peak, void* stream) {
  if (!wav || !pcm || !peak || rows < 0 || n < 0 || ld < n || (product != 0 && product != 1)) return fail("ctts_float_to_int16: bad arguments");
  CttsDeviceGuard dg(stream);
  CK(launch_float_to_int16(wav, n, ld, rows, per_row != 0, product, keep_thr, peak, pcm, keep_bits, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_float_to_int16_ragged(const float* wav, int16_t* pcm, uint8_t* keep_bits, const int64_t* off_dev, const int64_t* off_host,
                                          int32_t n_seg, int32_t product, float keep_thr, uint32_t* peak, void* stream) {
  if (!wav || !pcm || !peak || !off_dev || !off_host || n_seg < 1 || (product != 0 && product != 1))
    return fail("ctts_float_to_int16_ragged: bad arguments");
  if (off_host[0] != 0) return fail("ctts_float_to_int16_ragged: the first sample offset must be 0");
  long long n_max = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (off_host[i + 1] <= off_host[i]) return fail("ctts_float_to_int16_ragged: segment %d is empty or the offsets do not ascend", i);
    n_max = std::max(n_max, (long long)(off_host[i + 1] - off_host[i]));
  }
  CttsDeviceGuard dg(stream);
  CK(launch_float_to_int16_ragged(wav, (const long long*)off_dev, n_seg, n_max, product, keep_thr, peak, pcm, keep_bits, (hipStream_t)stream));
  return 0;
}
// tiles of 2048 samples (codec.hip, GT) of the longest group, per group: the size of the grouped conversion's count scratch
static long long groups_scratch_words(const int64_t* off_host, const int32_t* grp_host, int32_t n_grp, long long* n_max_out) {
  long long n_max = 0;
  for (int g = 0; g < n_grp; ++g) n_max = std::max(n_max, (long long)(off_host[grp_host[g + 1]] - off_host[grp_host[g]]));
  if (n_max_out) *n_max_out = n_max;
  return (long long)n_grp * ((n_max + 2047) / 2048);
}
static int groups_check(const char* who, const int64_t* off_host, int32_t n_seg, const int32_t* grp_host, int32_t n_grp) {
  if (!off_host || !grp_host) return fail("%s: bad arguments", who);
  if (n_grp < 1 || n_grp > 65535) return fail("%s: need 1 <= n_grp <= 65535 (got %d)", who, n_grp);
  if (n_seg < n_grp) return fail("%s: %d groups need at least as many segments (got %d)", who, n_grp, n_seg);
  if (off_host[0] != 0) return fail("%s: the first sample offset must be 0", who);
  for (int i = 0; i < n_seg; ++i)
    if (off_host[i + 1] <= off_host[i]) return fail("%s: segment %d is empty or the offsets do not ascend", who, i);
  if (grp_host[0] != 0 || grp_host[n_grp] != n_seg) return fail("%s: the group table must run from 0 to n_seg", who);
  for (int g = 0; g < n_grp; ++g) {
    if (grp_host[g + 1] <= grp_host[g]) return fail("%s: group %d is empty or the group table does not ascend", who, g);
    if (off_host[grp_host[g + 1]] - off_host[grp_host[g]] >= (1ll << 31)) return fail("%s: group %d holds 2^31 samples or more", who, g);
  }
  return 0;
}
extern "C" size_t ctts_float_to_int16_groups_scratch_bytes(const int64_t* off_host, int32_t n_seg, const int32_t* grp_host, int32_t n_grp) {
  if (groups_check("ctts_float_to_int16_groups_scratch_bytes", off_host, n_seg, grp_host, n_grp)) return 0;
  return (size_t)groups_scratch_words(off_host, grp_host, n_grp, nullptr) * sizeof(uint32_t);
}
extern "C" int ctts_float_to_int16_groups(const float* wav, int16_t* pcm, int64_t* n_kept, const int64_t* off_dev, const int64_t* off_host,
                                          int32_t n_seg, const int32_t* grp_dev, const int32_t* grp_host, int32_t n_grp, int32_t product,
                                          float keep_thr, uint32_t* peak, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "ctts_float_to_int16_groups";
  if (!wav || !pcm || !off_dev || !grp_dev || (product != 0 && product != 1)) return fail("%s: bad arguments", who);
  if (!peak || !n_kept) return fail("%s: the peak and count buffers must not be null", who);
  if (groups_check(who, off_host, n_seg, grp_host, n_grp)) return -1;
  if (((uintptr_t)pcm & 15) || ((uintptr_t)n_kept & 7)) return fail("%s: pcm must be 16-byte aligned, n_kept 8-byte aligned", who);
  long long n_max = 0;
  const long long words = groups_scratch_words(off_host, grp_host, n_grp, &n_max);
  if (!scratch || scratch_bytes < (size_t)words * sizeof(uint32_t)) return fail("%s: scratch too small (%zu bytes, need %lld)", who, scratch_bytes, words * 4);
  CttsDeviceGuard dg(stream);
  CK(launch_float_to_int16_groups(wav, (const long long*)off_dev, grp_dev, n_grp, n_max, product, keep_thr, peak, (unsigned*)scratch, pcm,
                                  (long long*)n_kept, (hipStream_t)stream));
  return 0;
}
extern "C" int32_t ctts_resample_supported(int32_t L, int32_t M, int32_t K) { return resample_mode(L, M, K); }
extern "C" int ctts_resample_ragged(const float* x, const int64_t* off_in_dev, const int64_t* off_in_host, float* y, const int64_t* off_out_dev,
                                    const int64_t* off_out_host, int32_t n_seg, const int32_t* sel_dev, const int32_t* sel_host, int32_t n_sel,
                                    const float* taps, int32_t L, int32_t M, int32_t K, void* stream) {
  const char* who = "ctts_resample_ragged";
  if (!x || !y || !off_in_dev || !off_in_host || !off_out_dev || !off_out_host || !taps || n_seg < 1) return fail("%s: bad arguments", who);
  if ((sel_dev == nullptr) != (sel_host == nullptr)) return fail("%s: the segment selection must be given on the device and the host, or on neither", who);
  if (L < 1 || M < 1 || L == M) return fail("%s: need L != M, both positive (got %d/%d)", who, L, M);
  if (resample_mode(L, M, K) == 0)
    return fail("%s: conversion %d/%d with %d taps is not supported (K = 2 width + M; a tile's input span within %d floats, the table within %d)",
                who, L, M, K, RS_LDS_FLOATS, RS_TAB_MAX);
  if (off_in_host[0] != 0 || off_out_host[0] != 0) return fail("%s: the first offsets must be 0", who);
  for (int i = 0; i < n_seg; ++i) {
    if (off_in_host[i + 1] <= off_in_host[i]) return fail("%s: segment %d is empty or the input offsets do not ascend", who, i);
    if (off_out_host[i + 1] <= off_out_host[i]) return fail("%s: segment %d's output is empty or the output offsets do not ascend", who, i);
  }
  if (off_out_host[n_seg] >= (1ll << 31)) return fail("%s: the output holds 2^31 samples or more", who);
  const int n_launch = sel_host ? n_sel : n_seg;
  if (n_launch < 1 || n_launch > 65535) return fail("%s: need 1 <= converted segments <= 65535 (got %d)", who, n_launch);
  long long n_out_max = 0;
  for (int q = 0; q < n_launch; ++q) {
    const int i = sel_host ? sel_host[q] : q;
    if (i < 0 || i >= n_seg) return fail("%s: selected segment %d is outside the pack", who, i);
    const long long n = off_in_host[i + 1] - off_in_host[i], no = off_out_host[i + 1] - off_out_host[i];
    if (n >= (1ll << 31) || no != (n * L + M - 1) / M) return fail("%s: segment %d: %lld samples in need ceil(n L / M) out, got %lld", who, i, n, no);
    n_out_max = std::max(n_out_max, no);
  }
  CttsDeviceGuard dg(stream);
  CK(launch_resample_ragged(x, (const long long*)off_in_dev, y, (const long long*)off_out_dev, sel_dev, n_launch, n_out_max, taps, L, M, K,
                            (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_time_scale_ragged(const float* x, const int64_t* off_in_dev, const int64_t* off_in_host, float* y, const int64_t* off_out_dev,
                                      const int64_t* off_out_host, int32_t* path, const int64_t* path_off_dev, const int64_t* path_off_host,
                                      int32_t n_seg, const float* window, int32_t num, int32_t den, void* stream) {
  const char* who = "ctts_time_scale_ragged";
  if (!x || !y || !path || !window || !off_in_dev || !off_in_host || !off_out_dev || !off_out_host || !path_off_dev || !path_off_host)
    return fail("%s: a null pointer (x, y, path, the window and the three offset tables on the device and the host are needed)", who);
  if (n_seg < 1 || n_seg > 65535) return fail("%s: need 1 <= n_seg <= 65535 (got %d)", who, n_seg);
  if (den != 100 || num < 50 || num > 200) return fail("%s: the speed is num / 100 with 50 <= num <= 200 (got %d/%d)", who, num, den);
  if (num == den) return fail("%s: speed 1 (%d/%d): there is nothing to scale", who, num, den);
  if (off_in_host[0] != 0 || off_out_host[0] != 0 || path_off_host[0] != 0) return fail("%s: the first offsets must be 0", who);
  long long n_out_max = 0;
  for (int i = 0; i < n_seg; ++i) {
    const long long n = off_in_host[i + 1] - off_in_host[i], no = off_out_host[i + 1] - off_out_host[i];
    if (n <= 0) return fail("%s: segment %d is empty or the input offsets do not ascend", who, i);
    if (no <= 0) return fail("%s: segment %d's output is empty or the output offsets do not ascend", who, i);
    // a frame reaches up to N + D samples past the end and the path is int32: keep every position below 2^31
    if (off_in_host[i + 1] >= (1ll << 31) - 4096) return fail("%s: the input holds 2^31 samples or more (less the 4096 a frame may reach past it)", who);
    if (no != (n * den + num - 1) / num) return fail("%s: segment %d: %lld samples in need ceil(n den / num) out, got %lld", who, i, n, no);
    if (path_off_host[i + 1] - path_off_host[i] != (no + TS_HS - 1) / TS_HS + 1)
      return fail("%s: segment %d: %lld samples out are ceil(n_out / %d) + 1 frames of path, got %lld", who, i, no, TS_HS,
                  (long long)(path_off_host[i + 1] - path_off_host[i]));
    n_out_max = std::max(n_out_max, no);
  }
  if (off_out_host[n_seg] >= (1ll << 31)) return fail("%s: the output holds 2^31 samples or more", who);
  CttsDeviceGuard dg(stream);
  CK(launch_time_scale_ragged(x, (const long long*)off_in_dev, y, (const long long*)off_out_dev, path, (const long long*)path_off_dev, n_seg,
                              n_out_max, window, num, den, (hipStream_t)stream));
  return 0;
}
// the sample offsets of a loudness call: 0 when they pass
static int loudness_offsets_check(const char* who, const int64_t* off_host, int32_t n_seg) {
  if (!off_host) return fail("%s: the host offsets are null", who);
  if (n_seg < 1 || n_seg > 65535) return fail("%s: need 1 <= n_seg <= 65535 (got %d)", who, n_seg);
  if (off_host[0] != 0) return fail("%s: the first sample offset must be 0", who);
  for (int i = 0; i < n_seg; ++i)
    if (off_host[i + 1] <= off_host[i]) return fail("%s: segment %d is empty or the offsets do not ascend", who, i);
  if (off_host[n_seg] >= (1ll << 31) - 4096) return fail("%s: the pack holds 2^31 - 4096 samples or more", who);
  return 0;
}
extern "C" size_t ctts_loudness_normalize_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg) {
  if (loudness_offsets_check("ctts_loudness_normalize_ragged_scratch_bytes", off_host, n_seg)) return 0;
  return (size_t)loudness_records(off_host[n_seg], n_seg) * LN_REC * sizeof(double) + (size_t)(n_seg + 3) / 4 * 16;
}
// both loudness entries; lim_dev / gain_out null: ctts_loudness_normalize_ragged
static int loudness_normalize_impl(const char* who, const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                   const int32_t* rate_dev, const int32_t* rate_host, const double* coef_dev, const double* coef_host,
                                   int32_t n_rates, const int32_t* grp_dev, const int32_t* grp_host, int32_t n_grp,
                                   const double* target_dev, const double* target_host, const int32_t* lim_dev, float* gain_out, void* stats,
                                   void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !y || !off_dev || !rate_dev || !rate_host || !coef_dev || !coef_host || !grp_dev || !grp_host || !target_dev || !target_host || !stats)
    return fail("%s: a null pointer (x, y, the stats and the offset, rate, coefficient, group and target tables on the device and the host are needed)", who);
  if (loudness_offsets_check(who, off_host, n_seg)) return -1;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)stats & 7)) return fail("%s: x and y must be 16-byte aligned, the stats 8-byte aligned", who);
  if (x != y && x < y + off_host[n_seg] && y < x + off_host[n_seg]) return fail("%s: y must be x itself or not overlap it", who);
  if (n_rates < 1) return fail("%s: the coefficient table is empty", who);
  for (int r = 0; r < n_rates; ++r) {
    const double H = coef_host[(size_t)r * LN_ROW], c = coef_host[(size_t)r * LN_ROW + 1];
    if (!(H >= LN_HMIN && H <= LN_HMAX) || H != (double)(int)H)
      return fail("%s: rate row %d: a sub-block of %g samples (the rate is a multiple of 10 Hz in %d .. %d)", who, r, H, 10 * LN_HMIN, 10 * LN_HMAX);
    if (c != (double)((((int)H + 63) / 64) | 1)) return fail("%s: rate row %d: the chunk is ceil(H / 64) | 1 samples (got %g for H = %g)", who, r, c, H);
  }
  long long n_max = 0, tiles_max = 0, h_max = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (rate_host[i] < 0 || rate_host[i] >= n_rates) return fail("%s: segment %d: rate row %d is outside the table of %d", who, i, rate_host[i], n_rates);
    const long long n = off_host[i + 1] - off_host[i], H = (long long)coef_host[(size_t)rate_host[i] * LN_ROW];
    n_max = std::max(n_max, n);
    tiles_max = std::max(tiles_max, (n + H - 1) / H);
    h_max = std::max(h_max, H);
  }
  if (n_grp < 1 || n_grp > n_seg) return fail("%s: need 1 <= n_grp <= n_seg (got %d groups, %d segments)", who, n_grp, n_seg);
  if (grp_host[0] != 0 || grp_host[n_grp] != n_seg) return fail("%s: the group table must run from 0 to n_seg", who);
  for (int g = 0; g < n_grp; ++g) {
    if (grp_host[g + 1] <= grp_host[g]) return fail("%s: group %d is empty or the group table does not ascend", who, g);
    const double t = target_host[g];
    if (t == t && !(t >= -40.0 && t <= -5.0)) return fail("%s: group %d: the target is -40 .. -5 LUFS, or NaN for none (got %g)", who, g, t);
  }
  const size_t rec_bytes = (size_t)loudness_records(off_host[n_seg], n_seg) * LN_REC * sizeof(double);
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < rec_bytes + (size_t)(n_seg + 3) / 4 * 16)
    return fail("%s: scratch missing, not 16-byte aligned or too small (%zu bytes, need %zu)", who, scratch_bytes, rec_bytes + (size_t)(n_seg + 3) / 4 * 16);
  CttsDeviceGuard dg(stream);
  CK(launch_loudness_normalize_ragged(x, y, (const long long*)off_dev, n_seg, n_max, tiles_max, (int)h_max, rate_dev, coef_dev, grp_dev, n_grp, target_dev,
                                      stats, (double*)scratch, (float*)((char*)scratch + rec_bytes), (hipStream_t)stream, lim_dev, gain_out));
  return 0;
}
extern "C" int ctts_loudness_normalize_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                              const int32_t* rate_dev, const int32_t* rate_host, const double* coef_dev, const double* coef_host,
                                              int32_t n_rates, const int32_t* grp_dev, const int32_t* grp_host, int32_t n_grp,
                                              const double* target_dev, const double* target_host, void* stats, void* scratch,
                                              size_t scratch_bytes, void* stream) {
  return loudness_normalize_impl("ctts_loudness_normalize_ragged", x, y, off_dev, off_host, n_seg, rate_dev, rate_host, coef_dev, coef_host, n_rates,
                                 grp_dev, grp_host, n_grp, target_dev, target_host, nullptr, nullptr, stats, scratch, scratch_bytes, stream);
}
extern "C" int ctts_loudness_limited_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                            const int32_t* rate_dev, const int32_t* rate_host, const double* coef_dev, const double* coef_host,
                                            int32_t n_rates, const int32_t* grp_dev, const int32_t* grp_host, int32_t n_grp,
                                            const double* target_dev, const double* target_host, const int32_t* lim_dev, const int32_t* lim_host,
                                            float* gain_out, void* stats, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "ctts_loudness_limited_ragged";
  if (!lim_dev || !lim_host || !gain_out) return fail("%s: a null pointer (the limiter table on the device and the host and the gains are needed)", who);
  if ((uintptr_t)gain_out & 3) return fail("%s: the gains must be 4-byte aligned", who);
  if (n_grp >= 1 && n_grp <= 65535)
    for (int g = 0; g < n_grp; ++g)
      if (lim_host[g] != 0 && lim_host[g] != 1) return fail("%s: group %d: the limiter flag is 0 or 1 (got %d)", who, g, lim_host[g]);
  return loudness_normalize_impl(who, x, y, off_dev, off_host, n_seg, rate_dev, rate_host, coef_dev, coef_host, n_rates, grp_dev, grp_host, n_grp,
                                 target_dev, target_host, lim_dev, gain_out, stats, scratch, scratch_bytes, stream);
}
extern "C" size_t ctts_peak_limit_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg) {
  if (loudness_offsets_check("ctts_peak_limit_ragged_scratch_bytes", off_host, n_seg)) return 0;
  return ((size_t)off_host[n_seg] * sizeof(float) + 15) / 16 * 16 + ((size_t)limiter_tiles(off_host[n_seg], n_seg) * sizeof(int32_t) + 15) / 16 * 16;
}
extern "C" int ctts_peak_limit_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                      const int32_t* rate_dev, const int32_t* rate_host, const float* gain_dev, void* stats, void* scratch,
                                      size_t scratch_bytes, void* stream) {
  const char* who = "ctts_peak_limit_ragged";
  if (!x || !y || !off_dev || !rate_dev || !rate_host || !gain_dev || !stats)
    return fail("%s: a null pointer (x, y, the gains, the stats and the offset and rate tables on the device and the host are needed)", who);
  if (loudness_offsets_check(who, off_host, n_seg)) return -1;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)stats & 3) || ((uintptr_t)gain_dev & 3))
    return fail("%s: x and y must be 16-byte aligned, the gains and the stats 4-byte aligned", who);
  if (x != y && x < y + off_host[n_seg] && y < x + off_host[n_seg]) return fail("%s: y must be x itself or not overlap it", who);
  long long n_max = 0;
  for (int i = 0; i < n_seg; ++i) {
    const int32_t fs = rate_host[i];
    if (fs < 100 * LM_WMIN || fs > 100 * LM_WMAX || fs % 10 != 0)
      return fail("%s: segment %d: the rate is a multiple of 10 Hz in %d .. %d (got %d)", who, i, 100 * LM_WMIN, 100 * LM_WMAX, fs);
    n_max = std::max(n_max, (long long)(off_host[i + 1] - off_host[i]));
  }
  const size_t curve_bytes = ((size_t)off_host[n_seg] * sizeof(float) + 15) / 16 * 16;
  const size_t need = curve_bytes + ((size_t)limiter_tiles(off_host[n_seg], n_seg) * sizeof(int32_t) + 15) / 16 * 16;
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need)
    return fail("%s: scratch missing, not 16-byte aligned or too small (%zu bytes, need %zu)", who, scratch_bytes, need);
  CttsDeviceGuard dg(stream);
  CK(launch_peak_limit_ragged(x, y, (const long long*)off_dev, n_seg, n_max, rate_dev, gain_dev, stats, (float*)scratch,
                              (int32_t*)((char*)scratch + curve_bytes), (hipStream_t)stream));
  return 0;
}
// ---- the dynamic range compressor: every table is checked on its host mirror before the first launch -----------------------------------
static_assert(sizeof(ctts_cp_stats) == 16 && CTTS_CP_TABLE == CP_TABLE, "ctts_cp_stats layout");
extern "C" size_t ctts_compress_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg) {
  if (loudness_offsets_check("ctts_compress_ragged_scratch_bytes", off_host, n_seg)) return 0;
  return ((size_t)compress_blocks(off_host[n_seg], n_seg) * sizeof(float) + 15) / 16 * 16;
}
extern "C" int ctts_compress_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                    const int32_t* rate_dev, const int32_t* rate_host, const int32_t* par_dev, const int32_t* par_host,
                                    const float* tab_dev, const float* tab_host, int32_t n_tab, void* stats, void* scratch,
                                    size_t scratch_bytes, void* stream) {
  const char* who = "ctts_compress_ragged";
  if (!x || !y || !off_dev || !rate_dev || !rate_host || !par_dev || !par_host || !tab_dev || !tab_host || !stats)
    return fail("%s: a null pointer (x, y, the stats and the offset, rate, parameter and gain tables on the device and the host are needed)", who);
  if (loudness_offsets_check(who, off_host, n_seg)) return -1;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)tab_dev & 15) || ((uintptr_t)stats & 3))
    return fail("%s: x, y and the gain tables must be 16-byte aligned, the stats 4-byte aligned", who);
  if (x != y && x < y + off_host[n_seg] && y < x + off_host[n_seg]) return fail("%s: y must be x itself or not overlap it", who);
  if (n_tab < 1 || n_tab > n_seg) return fail("%s: need 1 <= n_tab <= n_seg gain tables (got %d for %d segments)", who, n_tab, n_seg);
  for (int t = 0; t < n_tab; ++t)
    for (int q = 0; q < CP_TABLE; ++q) {
      const float g = tab_host[(size_t)t * CP_TABLE + q];
      if (!(g >= 0x1p-18f && g <= 1.0f)) return fail("%s: table %d: entry %d is a gain in 2^-18 .. 1 (got %g)", who, t, q, (double)g);
    }
  long long nb_max = 0;
  for (int i = 0; i < n_seg; ++i) {
    const int32_t fs = rate_host[i], A = par_host[4 * i], H = par_host[4 * i + 1], ti = par_host[4 * i + 2];
    if (fs < 1000 * CP_BMIN || fs > 1000 * CP_BMAX || fs % 10 != 0)
      return fail("%s: segment %d: the rate is a multiple of 10 Hz in %d .. %d (got %d)", who, i, 1000 * CP_BMIN, 1000 * CP_BMAX, fs);
    if (A < 1 || A > CP_AMAX) return fail("%s: segment %d: the attack is 1 .. %d blocks (got %d)", who, i, CP_AMAX, A);
    if (H < 0 || H > CP_HMAX) return fail("%s: segment %d: the hold is 0 .. %d blocks (got %d)", who, i, CP_HMAX, H);
    if (ti < -1 || ti >= n_tab) return fail("%s: segment %d: gain table %d is outside the %d given (-1: the segment is copied through)", who, i, ti, n_tab);
    const long long B = fs / 1000;
    nb_max = std::max(nb_max, (long long)(off_host[i + 1] - off_host[i] + B - 1) / B);
  }
  const size_t need = ((size_t)compress_blocks(off_host[n_seg], n_seg) * sizeof(float) + 15) / 16 * 16;
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need)
    return fail("%s: scratch missing, not 16-byte aligned or too small (%zu bytes, need %zu)", who, scratch_bytes, need);
  CttsDeviceGuard dg(stream);
  CK(launch_compress_ragged(x, y, (const long long*)off_dev, n_seg, nb_max, rate_dev, par_dev, tab_dev, stats, (float*)scratch,
                            (hipStream_t)stream));
  return 0;
}
// ---- the output equaliser: every table is checked on its host mirror before the first launch -------------------------------------------
static_assert(CTTS_EQ_ROW == EQ_ROW && CTTS_EQ_TILE == EQ_TILE, "the equaliser's table row and tile");
extern "C" size_t ctts_equalize_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg) {
  if (loudness_offsets_check("ctts_equalize_ragged_scratch_bytes", off_host, n_seg)) return 0;
  return (size_t)equalize_records(off_host[n_seg], n_seg) * EQ_D * sizeof(double);
}
extern "C" int ctts_equalize_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                    const int32_t* sel_dev, const int32_t* sel_host, const double* coef_dev, const double* coef_host,
                                    int32_t n_rows, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "ctts_equalize_ragged";
  if (!x || !y || !off_dev || !sel_dev || !sel_host || !coef_dev || !coef_host)
    return fail("%s: a null pointer (x, y and the offset, row index and coefficient tables on the device and the host are needed)", who);
  if (loudness_offsets_check(who, off_host, n_seg)) return -1;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)coef_dev & 15))
    return fail("%s: x, y and the coefficient table must be 16-byte aligned", who);
  if (x != y && x < y + off_host[n_seg] && y < x + off_host[n_seg]) return fail("%s: y must be x itself or not overlap it", who);
  if (n_rows < 1 || n_rows > n_seg) return fail("%s: need 1 <= n_rows <= n_seg coefficient rows (got %d for %d segments)", who, n_rows, n_seg);
  for (int r = 0; r < n_rows; ++r) {
    const double* R = coef_host + (size_t)r * EQ_ROW;
    if (!(R[0] >= 1.0 && R[0] <= (double)EQ_NSEC) || R[0] != (double)(int)R[0])
      return fail("%s: row %d: a cascade has 1 .. %d second-order sections (got %g)", who, r, EQ_NSEC, R[0]);
    if (!(R[1] >= 8000.0 && R[1] <= 48000.0) || R[1] != (double)(int)R[1] || (int)R[1] % 10 != 0)
      return fail("%s: row %d: the rate is a multiple of 10 Hz in 8000 .. 48000 (got %g)", who, r, R[1]);
    if (R[2] != (double)EQ_CHUNK) return fail("%s: row %d: the chunk is %d samples (got %g)", who, r, EQ_CHUNK, R[2]);
    const int ns = (int)R[0];
    for (int i = 0; i < ns; ++i) {
      const double* k = R + 4 + 5 * i;
      for (int q = 0; q < 5; ++q)
        if (!std::isfinite(k[q])) return fail("%s: row %d: section %d has a coefficient that is not finite", who, r, i);
      if (!(std::fabs(k[4]) < 1.0 && std::fabs(k[3]) < 1.0 + k[4]))
        return fail("%s: row %d: section %d is not stable (a1 = %g, a2 = %g)", who, r, i, k[3], k[4]);
    }
    for (int q = 32; q < 32 + 12 * EQ_D * EQ_D; ++q)
      if (!std::isfinite(R[q])) return fail("%s: row %d: a power of the state matrix is not finite", who, r);
  }
  long long tiles_max = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (sel_host[i] < -1 || sel_host[i] >= n_rows)
      return fail("%s: segment %d: coefficient row %d is outside the %d given (-1: the segment is copied through)", who, i, sel_host[i], n_rows);
    tiles_max = std::max(tiles_max, (long long)(off_host[i + 1] - off_host[i] + EQ_TILE - 1) / EQ_TILE);
  }
  const size_t need = (size_t)equalize_records(off_host[n_seg], n_seg) * EQ_D * sizeof(double);
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need)
    return fail("%s: scratch missing, not 16-byte aligned or too small (%zu bytes, need %zu)", who, scratch_bytes, need);
  CttsDeviceGuard dg(stream);
  CK(launch_equalize_ragged(x, y, (const long long*)off_dev, n_seg, tiles_max, sel_dev, coef_dev, (double*)scratch, (hipStream_t)stream));
  return 0;
}
// ---- the limiter of streams: the host's arithmetic (limiter.py: stream_plan) and every check the launch trusts --------------------------
static_assert(sizeof(ctts_lm_stream) == 80 && sizeof(LmStream) == 80 && offsetof(ctts_lm_stream, n_out) == offsetof(LmStream, n_out) &&
              offsetof(ctts_lm_stream, slot) == offsetof(LmStream, slot) && offsetof(ctts_lm_stream, c_out) == offsetof(LmStream, c_out) &&
              offsetof(ctts_lm_stream, rate) == offsetof(LmStream, rate) && offsetof(ctts_lm_stream, gain) == offsetof(LmStream, gain) &&
              CTTS_LM_CARRY == LM_CARRY, "ctts_lm_stream layout");
extern "C" int ctts_peak_limit_stream_step(const float* x, int64_t n_x, const ctts_lm_stream* st_dev, const ctts_lm_stream* st_host,
                                           int32_t n_streams, float* y, int64_t n_y, float* carry, void* stats, int32_t n_slots, void* stream) {
  const char* who = "ctts_peak_limit_stream_step";
  if (!st_dev || !st_host || !carry || !stats) return fail("%s: a null pointer (both descriptor tables, the carry and the stats are needed)", who);
  if (n_x < 0 || n_y < 0 || (!x && n_x) || (!y && n_y)) return fail("%s: a null pointer (x or y) with a length other than 0", who);
  if (n_streams < 1 || n_streams > 1024) return fail("%s: need 1 <= n_streams <= 1024 (got %d)", who, n_streams);
  if (n_slots < 1) return fail("%s: the state pool has no slot", who);
  if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)carry & 3) || ((uintptr_t)stats & 3))
    return fail("%s: x, y, the carry and the stats must be 4-byte aligned", who);
  if (n_x && n_y && x < y + n_y && y < x + n_x) return fail("%s: y must not overlap x (a stream is never limited in place)", who);
  std::vector<char> seen((size_t)n_slots, 0);
  long long n_out_max = 0;
  int reset = 0;
  for (int i = 0; i < n_streams; ++i) {
    const ctts_lm_stream& w = st_host[i];
    if (w.slot < 0 || w.slot >= n_slots) return fail("%s: limiter stream %d: slot %d is outside the pool of %d", who, i, w.slot, n_slots);
    if (seen[w.slot]) return fail("%s: limiter stream %d: slot %d appears twice in one launch", who, i, w.slot);
    seen[w.slot] = 1;
    if (w.phase != 0 && w.phase != 1) return fail("%s: limiter stream %d: phase %d is neither 0 nor 1", who, i, w.phase);
    if (w.rate < 100 * LM_WMIN || w.rate > 100 * LM_WMAX || w.rate % 10 != 0)
      return fail("%s: limiter stream %d: the rate is a multiple of 10 Hz in %d .. %d (got %d)", who, i, 100 * LM_WMIN, 100 * LM_WMAX, w.rate);
    if (!(w.gain > 0.0f) || !std::isfinite(w.gain)) return fail("%s: limiter stream %d: the pre-gain is a positive finite number", who, i);
    if (w.n_in < 0 || w.pos < 0 || w.in_off < 0 || w.out_off < 0 || w.e_lo < 0 || w.n_out < 0)
      return fail("%s: limiter stream %d: a negative length, position or offset", who, i);
    if (w.pos >= (1ll << 31) || w.n_in >= (1ll << 31) || w.pos + w.n_in >= (1ll << 31))
      return fail("%s: limiter stream %d would hold 2^31 samples or more", who, i);
    if (w.in_off + w.n_in > n_x) return fail("%s: limiter stream %d: the push lies outside the input (%lld floats)", who, i, (long long)n_x);
    const long long W = w.rate / 100, end = w.pos + w.n_in;
    const bool fin = w.total != -1;
    if (fin && w.total != end)
      return fail("%s: limiter stream %d: a last push ends the stream at pos + n_in = %lld, got total %lld", who, i, end, (long long)w.total);
    const long long e0 = std::max(0ll, w.pos - 2 * W), e1 = fin ? end : std::max(0ll, end - 2 * W);
    if (w.e_lo != e0) return fail("%s: limiter stream %d: %lld samples have emitted %lld, got e_lo %lld", who, i, (long long)w.pos, e0, (long long)w.e_lo);
    if (w.n_out != e1 - e0) return fail("%s: limiter stream %d: the step emits %lld samples, got %lld", who, i, e1 - e0, (long long)w.n_out);
    if (w.out_off + w.n_out > n_y) return fail("%s: limiter stream %d: the chunk lies outside the output (%lld floats)", who, i, (long long)n_y);
    const long long c_in = std::min((long long)w.pos, 4 * W), c_out = fin ? 0 : std::min(end, 4 * W);
    if (w.c_in != c_in || w.c_out != c_out)
      return fail("%s: limiter stream %d: the step carries %lld samples in and %lld out, got %d and %d", who, i, c_in, c_out, w.c_in, w.c_out);
    n_out_max = std::max(n_out_max, (long long)w.n_out);
    reset |= w.pos == 0;
  }
  CttsDeviceGuard dg(stream);
  CK(launch_peak_limit_stream(x, (const LmStream*)st_dev, n_streams, n_out_max, y, carry, stats, reset, (hipStream_t)stream));
  return 0;
}
// ---- the compressor of streams: the host's arithmetic (compressor.py: stream_plan) and every check the launches trust ------------------
static_assert(sizeof(ctts_cp_stream) == 104 && sizeof(CpStream) == 104 && offsetof(ctts_cp_stream, cb_off) == offsetof(CpStream, cb_off) &&
              offsetof(ctts_cp_stream, slot) == offsetof(CpStream, slot) && offsetof(ctts_cp_stream, rate) == offsetof(CpStream, rate) &&
              offsetof(ctts_cp_stream, tab) == offsetof(CpStream, tab) && offsetof(ctts_cp_stream, c_in) == offsetof(CpStream, c_in) &&
              offsetof(ctts_cp_stream, h_out) == offsetof(CpStream, h_out) && CTTS_CP_SCARRY == CP_SCARRY && CTTS_CP_SHIST == CP_SHIST,
              "ctts_cp_stream layout");
extern "C" size_t ctts_compress_stream_scratch_bytes(int64_t n_blocks) {
  if (n_blocks < 0 || n_blocks >= (1ll << 31)) return 0;
  return ((size_t)std::max<int64_t>(n_blocks, 4) * sizeof(float) + 15) / 16 * 16;
}
extern "C" int ctts_compress_stream_step(const float* x, int64_t n_x, const ctts_cp_stream* st_dev, const ctts_cp_stream* st_host,
                                         int32_t n_streams, const float* tab_dev, const float* tab_host, int32_t n_tab, float* y, int64_t n_y,
                                         float* carry, float* hold, void* stats, int32_t n_slots, void* scratch, size_t scratch_bytes,
                                         void* stream) {
  const char* who = "ctts_compress_stream_step";
  if (!st_dev || !st_host || !tab_dev || !tab_host || !carry || !hold || !stats || !scratch)
    return fail("%s: a null pointer (both descriptor tables, the gain tables on the device and the host, the carry, the hold, the stats and the scratch are needed)", who);
  if (n_x < 0 || n_y < 0 || (!x && n_x) || (!y && n_y)) return fail("%s: a null pointer (x or y) with a length other than 0", who);
  if (n_streams < 1 || n_streams > 1024) return fail("%s: need 1 <= n_streams <= 1024 (got %d)", who, n_streams);
  if (n_slots < 1) return fail("%s: the state pool has no slot", who);
  if (((uintptr_t)x & 15) || ((uintptr_t)tab_dev & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)y & 3) || ((uintptr_t)carry & 3) ||
      ((uintptr_t)hold & 3) || ((uintptr_t)stats & 3))
    return fail("%s: x, the gain tables and the scratch must be 16-byte aligned, y, the carry, the hold and the stats 4-byte aligned", who);
  if (n_x && n_y && x < y + n_y && y < x + n_x) return fail("%s: y must not overlap x (a stream is never compressed in place)", who);
  if (n_tab < 1 || n_tab > n_streams) return fail("%s: need 1 <= n_tab <= n_streams gain tables (got %d for %d streams)", who, n_tab, n_streams);
  for (int t = 0; t < n_tab; ++t)
    for (int q = 0; q < CP_TABLE; ++q) {
      const float g = tab_host[(size_t)t * CP_TABLE + q];
      if (!(g >= 0x1p-18f && g <= 1.0f)) return fail("%s: table %d: entry %d is a gain in 2^-18 .. 1 (got %g)", who, t, q, (double)g);
    }
  std::vector<char> seen((size_t)n_slots, 0);
  long long nb_new_max = 0, nb_out_max = 0, cb = 0;
  for (int i = 0; i < n_streams; ++i) {
    const ctts_cp_stream& w = st_host[i];
    if (w.slot < 0 || w.slot >= n_slots) return fail("%s: compressor stream %d: slot %d is outside the pool of %d", who, i, w.slot, n_slots);
    if (seen[w.slot]) return fail("%s: compressor stream %d: slot %d appears twice in one launch", who, i, w.slot);
    seen[w.slot] = 1;
    if (w.phase != 0 && w.phase != 1) return fail("%s: compressor stream %d: phase %d is neither 0 nor 1", who, i, w.phase);
    if (w.rate < 1000 * CP_BMIN || w.rate > 1000 * CP_BMAX || w.rate % 10 != 0)
      return fail("%s: compressor stream %d: the rate is a multiple of 10 Hz in %d .. %d (got %d)", who, i, 1000 * CP_BMIN, 1000 * CP_BMAX, w.rate);
    if (w.A < 1 || w.A > CP_AMAX) return fail("%s: compressor stream %d: the attack is 1 .. %d blocks (got %d)", who, i, CP_AMAX, w.A);
    if (w.H < 0 || w.H > CP_HMAX) return fail("%s: compressor stream %d: the hold is 0 .. %d blocks (got %d)", who, i, CP_HMAX, w.H);
    if (w.tab < 0 || w.tab >= n_tab) return fail("%s: compressor stream %d: gain table %d is outside the %d given", who, i, w.tab, n_tab);
    if (w.n_in < 0 || w.pos < 0 || w.in_off < 0 || w.out_off < 0 || w.e_lo < 0 || w.n_out < 0)
      return fail("%s: compressor stream %d: a negative length, position or offset", who, i);
    if (w.pos >= (1ll << 31) || w.n_in >= (1ll << 31) || w.pos + w.n_in >= (1ll << 31))
      return fail("%s: compressor stream %d would hold 2^31 samples or more", who, i);
    if (w.in_off + w.n_in > n_x) return fail("%s: compressor stream %d: the push lies outside the input (%lld floats)", who, i, (long long)n_x);
    const long long B = w.rate / 1000, end = w.pos + w.n_in, reach = w.A + w.H + 1;
    const bool fin = w.total != -1;
    if (fin && w.total != end)
      return fail("%s: compressor stream %d: a last push ends the stream at pos + n_in = %lld, got total %lld", who, i, end, (long long)w.total);
    const long long nbc0 = w.pos / B, nbc1 = fin ? (end + B - 1) / B : end / B;
    const long long e0 = std::max(0ll, nbc0 - w.A - 1) * B, e1 = fin ? end : std::max(0ll, end / B - w.A - 1) * B;
    if (w.e_lo != e0) return fail("%s: compressor stream %d: %lld samples have emitted %lld, got e_lo %lld", who, i, (long long)w.pos, e0, (long long)w.e_lo);
    if (w.n_out != e1 - e0) return fail("%s: compressor stream %d: the step emits %lld samples, got %lld", who, i, e1 - e0, (long long)w.n_out);
    if (w.out_off + w.n_out > n_y) return fail("%s: compressor stream %d: the chunk lies outside the output (%lld floats)", who, i, (long long)n_y);
    const long long c_in = w.pos - e0, c_out = fin ? 0 : end - e1;
    const long long h_in = nbc0 - std::max(0ll, e0 / B - reach), h_out = fin ? 0 : nbc1 - std::max(0ll, e1 / B - reach);
    if (w.c_in != c_in || w.c_out != c_out)
      return fail("%s: compressor stream %d: the step carries %lld samples in and %lld out, got %d and %d", who, i, c_in, c_out, w.c_in, w.c_out);
    if (w.h_in != h_in || w.h_out != h_out)
      return fail("%s: compressor stream %d: the step carries %lld block gains in and %lld out, got %d and %d", who, i, h_in, h_out, w.h_in, w.h_out);
    if (c_in > CP_SCARRY || c_out > CP_SCARRY || h_in > CP_SHIST || h_out > CP_SHIST)       // cannot be, by the ranges above
      return fail("%s: compressor stream %d: the carry does not fit its slot", who, i);
    if (w.cb_off != cb) return fail("%s: compressor stream %d: its new block gains start at float %lld of the scratch, got %lld", who, i, cb, (long long)w.cb_off);
    cb += nbc1 - nbc0;
    nb_new_max = std::max(nb_new_max, nbc1 - nbc0);
    nb_out_max = std::max(nb_out_max, (e1 - e0 + B - 1) / B);
  }
  const size_t need = ctts_compress_stream_scratch_bytes(cb);
  if (need == 0 || scratch_bytes < need) return fail("%s: scratch too small (%zu bytes, need %zu)", who, scratch_bytes, need);
  CttsDeviceGuard dg(stream);
  CK(launch_compress_stream(x, (const CpStream*)st_dev, n_streams, nb_new_max, nb_out_max, tab_dev, y, carry, hold, stats, (float*)scratch,
                            (hipStream_t)stream));
  return 0;
}
extern "C" size_t ctts_trim_pauses_ragged_scratch_bytes(int64_t frames, int32_t n_seg) {
  if (frames < 1 || frames >= (1ll << 31) || n_seg < 1 || n_seg > 65535) return 0;
  return pause_scratch_bytes(frames, n_seg);
}
extern "C" int ctts_trim_pauses_ragged(const float* in, float* out, const int64_t* off_dev, const int64_t* off_host, const int64_t* fbase_dev,
                                       const int64_t* fbase_host, const int32_t* rows_dev, const int32_t* rows_host, int32_t n_seg,
                                       const float* fade_dev, int32_t n_fade, int64_t* off_out, int32_t* records, void* scratch,
                                       size_t scratch_bytes, void* stream) {
  const char* who = "ctts_trim_pauses_ragged";
  if (!in || !out || !off_dev || !off_host || !fbase_dev || !fbase_host || !rows_dev || !rows_host || !fade_dev || !off_out || !records || !scratch)
    return fail("%s: a null pointer (in, out, the offset, frame base and row tables on the device and the host, the fade table, off_out, the records and the scratch are needed)", who);
  if (loudness_offsets_check(who, off_host, n_seg)) return -1;
  const long long total = off_host[n_seg];
  if (((uintptr_t)in & 15) || ((uintptr_t)out & 15) || ((uintptr_t)off_out & 7) || ((uintptr_t)records & 3) || ((uintptr_t)scratch & 15))
    return fail("%s: in, out and the scratch must be 16-byte aligned, off_out 8-byte, the records 4-byte", who);
  if (in < out + total && out < in + total) return fail("%s: out must not overlap in", who);
  if (n_fade < 0) return fail("%s: the fade table's length is negative", who);
  if (fbase_host[0] != 0) return fail("%s: the first frame base must be 0", who);
  long long frames_max = 0;
  for (int i = 0; i < n_seg; ++i) {
    const int32_t* r = rows_host + (size_t)i * PA_ROW;
    const long long n = off_host[i + 1] - off_host[i];
    if (r[0] < PA_FMIN || r[0] > PA_FMAX) return fail("%s: segment %d: a frame of %d samples (the rate is %d .. %d Hz)", who, i, r[0], 100 * PA_FMIN, 100 * PA_FMAX);
    if (r[4] < 0 || r[4] > 1000 || r[1] < 0 || r[1] > 100 || r[2] < 0 || r[2] > 1000 || r[3] < 0 || r[3] > 1000)
      return fail("%s: segment %d: pad 0 .. 100, lead and tail 0 .. 1000, P 0 (copy) .. 1000 frames (got %d, %d, %d, %d)", who, i, r[1], r[2], r[3], r[4]);
    if (r[4] != 0) {
      float thr;
      memcpy(&thr, r + 5, 4);
      if (!(thr >= 9e-6f && thr <= 1.0f)) return fail("%s: segment %d: the threshold is -100 .. 0 dB (got an amplitude of %g)", who, i, (double)thr);
      if (r[6] < 0 || (long long)r[6] + r[0] > n_fade) return fail("%s: segment %d: its fade table [%d, %d) lies outside the %d floats given", who, i, r[6], r[6] + r[0], n_fade);
    }
    const long long nf = (n + r[0] - 1) / r[0];
    if (fbase_host[i + 1] - fbase_host[i] != nf)
      return fail("%s: segment %d: %lld samples in frames of %d are %lld frames, the frame bases say %lld", who, i, n, r[0], nf, (long long)(fbase_host[i + 1] - fbase_host[i]));
    frames_max = std::max(frames_max, nf);
  }
  const long long frames = fbase_host[n_seg];
  if (scratch_bytes < pause_scratch_bytes(frames, n_seg))
    return fail("%s: scratch too small (%zu bytes, need %zu)", who, scratch_bytes, pause_scratch_bytes(frames, n_seg));
  CttsDeviceGuard dg(stream);
  CK(launch_trim_pauses_ragged(in, out, (const long long*)off_dev, (const long long*)fbase_dev, rows_dev, n_seg, frames_max, frames, fade_dev,
                               (long long*)off_out, records, scratch, (hipStream_t)stream));
  return 0;
}
// ---- pause control of streams: the host's arithmetic (pauses.py: stream_need and the step's layout) and every check the launches trust ----
static_assert(sizeof(ctts_pa_stream) == 96 && sizeof(PaStream) == 96 && offsetof(ctts_pa_stream, list_off) == offsetof(PaStream, list_off) &&
              offsetof(ctts_pa_stream, slot) == offsetof(PaStream, slot) && offsetof(ctts_pa_stream, fin) == offsetof(PaStream, fin) &&
              offsetof(ctts_pa_stream, P) == offsetof(PaStream, P) && offsetof(ctts_pa_stream, thr) == offsetof(PaStream, thr) &&
              offsetof(ctts_pa_stream, n_list) == offsetof(PaStream, n_list) && CTTS_PA_STREAM_FRAMES == PA_SCAP &&
              CTTS_PA_STREAM_CARRY == PA_SCARRY && CTTS_PA_STREAM_STATE == PA_STATE && CTTS_PA_STREAM_RES == PA_RES, "ctts_pa_stream layout");
// pauses.stream_need in frames
static long long pause_stream_need(long long P, long long lead, long long tail, long long pad) {
  const long long h = (P + 1) / 2, t = P - h, k0 = std::min(h - 1, tail);
  return std::max(std::max(std::max(1ll, lead + tail) + lead + pad, P + pad - k0), std::max(h, tail) - k0 + t + 1 + pad);
}
extern "C" size_t ctts_trim_pauses_stream_scratch_bytes(int64_t frames, int64_t entries) {
  if (frames < 0 || frames >= (1ll << 31) || entries < 1 || entries >= (1ll << 31)) return 0;
  return pause_stream_scratch_bytes(frames, entries);
}
extern "C" int ctts_trim_pauses_stream_step(const float* x, int64_t n_x, const ctts_pa_stream* st_dev, const ctts_pa_stream* st_host,
                                            int32_t n_streams, float* y, int64_t n_y, float* carry, int32_t* state, int32_t n_slots,
                                            const float* fade_dev, int32_t n_fade, int32_t* res, void* scratch, size_t scratch_bytes,
                                            void* stream) {
  const char* who = "ctts_trim_pauses_stream_step";
  if (!st_dev || !st_host || !carry || !state || !fade_dev || !res || !scratch)
    return fail("%s: a null pointer (both descriptor tables, the carry, the state, the fade table, the results and the scratch are needed)", who);
  if (n_x < 0 || n_y < 0 || (!x && n_x) || (!y && n_y)) return fail("%s: a null pointer (x or y) with a length other than 0", who);
  if (n_streams < 1 || n_streams > 1024) return fail("%s: need 1 <= n_streams <= 1024 (got %d)", who, n_streams);
  if (n_slots < 1) return fail("%s: the state pool has no slot", who);
  if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)carry & 3) || ((uintptr_t)state & 3) || ((uintptr_t)fade_dev & 3) || ((uintptr_t)res & 3) ||
      ((uintptr_t)scratch & 15))
    return fail("%s: x, y, the carry, the state, the fade table and the results must be 4-byte aligned, the scratch 16-byte", who);
  if (n_x && n_y && x < y + n_y && y < x + n_x) return fail("%s: y must not overlap x (a stream is never trimmed in place)", who);
  if (n_fade < 0) return fail("%s: the fade table's length is negative", who);
  std::vector<char> seen((size_t)n_slots, 0);
  long long frames = 0, entries = 0, nf_max = 0, list_max = 0;
  for (int i = 0; i < n_streams; ++i) {
    const ctts_pa_stream& w = st_host[i];
    if (w.slot < 0 || w.slot >= n_slots) return fail("%s: pause stream %d: slot %d is outside the pool of %d", who, i, w.slot, n_slots);
    if (seen[w.slot]) return fail("%s: pause stream %d: slot %d appears twice in one launch", who, i, w.slot);
    seen[w.slot] = 1;
    if (w.phase != 0 && w.phase != 1) return fail("%s: pause stream %d: phase %d is neither 0 nor 1", who, i, w.phase);
    if (w.fin != 0 && w.fin != 1) return fail("%s: pause stream %d: the last-push flag is 0 or 1 (got %d)", who, i, w.fin);
    if (w.F < PA_FMIN || w.F > PA_FMAX) return fail("%s: pause stream %d: a frame of %d samples (the rate is %d .. %d Hz)", who, i, w.F, 100 * PA_FMIN, 100 * PA_FMAX);
    if (w.P < 1 || w.P > 1000 || w.pad < 0 || w.pad > 100 || w.lead < 0 || w.lead > 1000 || w.tail < 0 || w.tail > 1000)
      return fail("%s: pause stream %d: pad 0 .. 100, lead and tail 0 .. 1000, P 1 .. 1000 frames (got %d, %d, %d, %d)", who, i, w.pad, w.lead, w.tail, w.P);
    if (!(w.thr >= 9e-6f && w.thr <= 1.0f)) return fail("%s: pause stream %d: the threshold is -100 .. 0 dB (got an amplitude of %g)", who, i, (double)w.thr);
    if (w.fade < 0 || (long long)w.fade + w.F > n_fade)
      return fail("%s: pause stream %d: its fade table [%d, %d) lies outside the %d floats given", who, i, w.fade, w.fade + w.F, n_fade);
    const long long need = pause_stream_need(w.P, w.lead, w.tail, w.pad);
    if (need > PA_SCAP) return fail("%s: pause stream %d: this spec makes a stream hold %lld frames, a slot holds %d", who, i, need, PA_SCAP);
    if (w.need != need) return fail("%s: pause stream %d: this spec needs %lld frames, got %d", who, i, need, w.need);
    if (w.n_in < 0 || w.pos < 0 || w.in_off < 0 || w.out_off < 0) return fail("%s: pause stream %d: a negative length, position or offset", who, i);
    if (w.pos >= (1ll << 31) || w.n_in >= (1ll << 31) || w.pos + w.n_in >= (1ll << 31))
      return fail("%s: pause stream %d would hold 2^31 samples or more", who, i);
    if (w.in_off + w.n_in > n_x) return fail("%s: pause stream %d: the push lies outside the input (%lld floats)", who, i, (long long)n_x);
    const long long avail = w.pos % w.F + w.n_in, nf = avail / w.F + (w.fin && avail % w.F ? 1 : 0), room = need * w.F + avail;
    if (room >= (1ll << 31)) return fail("%s: pause stream %d: the chunk could hold 2^31 samples or more", who, i);
    if (w.out_off + room > n_y)
      return fail("%s: pause stream %d: the chunk's room (%lld floats: what may wait and what arrives) lies outside the output (%lld floats)", who, i, room, (long long)n_y);
    const long long nl = 2 * need + nf + 1;
    if (w.fr_off != frames || w.list_off != entries || w.n_list != nl)
      return fail("%s: pause stream %d: its new frames start at %lld and its copy list is [%lld, +%lld), got %lld and [%lld, +%d)", who, i, frames, entries, nl,
                  (long long)w.fr_off, (long long)w.list_off, w.n_list);
    frames += nf;
    entries += nl;
    nf_max = std::max(nf_max, nf);
    list_max = std::max(list_max, nl);
  }
  if (frames >= (1ll << 31) || entries >= (1ll << 31)) return fail("%s: 2^31 frames or copy-list entries in one step", who);
  for (int i = 0; i < n_streams; ++i)                             // chunks may not share room: a step's output length is known only on the device
    for (int k = 0; k < i; ++k) {
      const ctts_pa_stream &a = st_host[i], &b = st_host[k];
      const long long ra = (long long)a.need * a.F + a.pos % a.F + a.n_in, rb = (long long)b.need * b.F + b.pos % b.F + b.n_in;
      if (a.out_off < b.out_off + rb && b.out_off < a.out_off + ra) return fail("%s: pause streams %d and %d: the chunks' rooms overlap", who, k, i);
    }
  if (scratch_bytes < pause_stream_scratch_bytes(frames, entries))
    return fail("%s: scratch too small (%zu bytes, need %zu)", who, scratch_bytes, pause_stream_scratch_bytes(frames, entries));
  CttsDeviceGuard dg(stream);
  CK(launch_trim_pauses_stream(x, (const PaStream*)st_dev, n_streams, nf_max, list_max, frames, y, carry, state, fade_dev, res, scratch,
                               (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_copy_bytes(void* dst,const void* src, size_t bytes, void* stream) {
  if (!dst || !src || (bytes & 15) || (((uintptr_t)dst | (uintptr_t)src) & 15)) return fail("ctts_copy_bytes: pointers and size must be 16-byte aligned");
  CttsDeviceGuard dg(stream);
  CK(launch_copy16(src, dst, bytes, (hipStream_t)stream));
  return 0;
}
static_assert(sizeof(ctts_g711_range) == 32 && sizeof(G711Range) == 32 && offsetof(ctts_g711_range, law) == offsetof(G711Range, law) &&
              offsetof(ctts_g711_range, n) == offsetof(G711Range, n), "ctts_g711_range layout");
extern "C" int ctts_g711_encode_ranges(const int16_t* pcm, uint8_t* out, const ctts_g711_range* rng_dev, const ctts_g711_range* rng_host,
                                       int32_t n_rng, void* stream) {
  const char* who = "ctts_g711_encode_ranges";
  if (!pcm || !out || !rng_dev || !rng_host) return fail("%s: a null pointer (pcm, out and both range tables are needed)", who);
  if (n_rng < 1 || n_rng > 1024) return fail("%s: need 1 <= n_rng <= 1024 (got %d)", who, n_rng);
  if (((uintptr_t)pcm & 15) || ((uintptr_t)out & 15)) return fail("%s: pcm and out must be 16-byte aligned", who);
  long long end = 0, n_max = 0;
  for (int i = 0; i < n_rng; ++i) {
    const ctts_g711_range& r = rng_host[i];
    if (r.law < -1 || r.law > 1) return fail("%s: range %d: law %d is none of -1 (skip), 0 (mu-law), 1 (A-law)", who, i, r.law);
    if (r.start < 0 || (r.start & 7)) return fail("%s: range %d starts at element %lld: starts are multiples of 8", who, i, (long long)r.start);
    if (r.n < 0) return fail("%s: range %d has a negative length (%lld)", who, i, (long long)r.n);
    if (r.start >= (1ll << 46) || r.n >= (1ll << 40)) return fail("%s: range %d lies beyond what a launch can address", who, i);
    if (r.start < end) return fail("%s: range %d starts at element %lld, before the end %lld of the ranges in front of it (overlapping or descending)", who,
                                   i, (long long)r.start, end);
    end = r.start + r.n;
    if (r.law >= 0) n_max = std::max(n_max, (long long)r.n);
  }
  const uintptr_t p0 = (uintptr_t)pcm, o0 = (uintptr_t)out;
  if (p0 == o0 || (p0 < o0 + (uintptr_t)end && o0 < p0 + 2 * (uintptr_t)end))
    return fail("%s: out aliases pcm (the conversion is not in place)", who);
  if (n_max == 0) return 0;                      // nothing but skipped or empty ranges
  CttsDeviceGuard dg(stream);
  CK(launch_g711_ranges(pcm, out, (const G711Range*)rng_dev, n_rng, n_max, (hipStream_t)stream));
  return 0;
}
static_assert(sizeof(ctts_flac_range) == 32 && sizeof(FlacRange) == 32 && offsetof(ctts_flac_range, rate) == offsetof(FlacRange, rate) &&
              offsetof(ctts_flac_range, count_idx) == offsetof(FlacRange, count_idx) &&
              offsetof(ctts_flac_range, frame0) == offsetof(FlacRange, frame0) && sizeof(FlacFrame) == 96, "ctts_flac_range layout");
static bool flac_rate_ok(int32_t rate) {
  switch (rate) {
    case 88200: case 176400: case 192000: case 96000: return true;
  }
  return rate >= 1 && rate <= 65535;
}
// the checks of a host table; sizes: n_frames, out bytes, work bytes, the most slots of one range, the end of the last range (elements)
static int flac_check_table(const char* who, const ctts_flac_range* rng_host, int32_t n_rng, long long sizes[5], bool* wants_counts) {
  if (!rng_host) return fail("%s: a null pointer (the host range table is needed)", who);
  if (n_rng < 1 || n_rng > 1024) return fail("%s: need 1 <= n_rng <= 1024 (got %d)", who, n_rng);
  long long end = 0, frames = 0, frames_max = 0, out_bytes = 0;
  *wants_counts = false;
  for (int i = 0; i < n_rng; ++i) {
    const ctts_flac_range& r = rng_host[i];
    if (r.rate != 0 && !flac_rate_ok(r.rate))
      return fail("%s: range %d: a rate of %d Hz cannot be coded (0 skips the range; else a rate of the format's table or 1 .. 65535)", who, i, r.rate);
    if (r.start < 0 || (r.start & 7)) return fail("%s: range %d starts at element %lld: starts are multiples of 8", who, i, (long long)r.start);
    if (r.n < 0) return fail("%s: range %d has a negative length (%lld)", who, i, (long long)r.n);
    if (r.start >= (1ll << 46) || r.n >= (1ll << 31)) return fail("%s: range %d lies beyond what a launch can address (n < 2^31)", who, i);
    if (r.start < end) return fail("%s: range %d starts at element %lld, before the end %lld of the ranges in front of it (overlapping or descending)", who,
                                   i, (long long)r.start, end);
    if (r.count_idx < -1 || r.count_idx > 65535) return fail("%s: range %d: count_idx %d is neither -1 nor in 0 .. 65535", who, i, r.count_idx);
    end = r.start + r.n;
    if (r.frame0 != frames) return fail("%s: range %d: frame0 is %lld, the ranges in front of it own %lld frame slots", who, i, (long long)r.frame0, frames);
    if (r.rate == 0) continue;
    if (r.count_idx >= 0) *wants_counts = true;
    const long long fr = (r.n + FLAC_BLOCK - 1) / FLAC_BLOCK;
    frames += fr;
    frames_max = std::max(frames_max, fr);
    out_bytes += 2 * r.n + 16 * fr;
  }
  sizes[0] = frames;
  sizes[1] = out_bytes;
  sizes[2] = ((frames + 1 + n_rng) * 8 + frames * (long long)sizeof(FlacFrame) + 15) / 16 * 16;
  sizes[3] = frames_max;
  sizes[4] = end;
  return 0;
}
extern "C" int ctts_flac_encode_sizes(const ctts_flac_range* rng_host, int32_t n_rng, int64_t* sizes) {
  const char* who = "ctts_flac_encode_sizes";
  if (!sizes) return fail("%s: a null pointer (sizes[3] is needed)", who);
  long long s[5];
  bool wants_counts;
  if (flac_check_table(who, rng_host, n_rng, s, &wants_counts)) return -1;
  sizes[0] = s[0];
  sizes[1] = s[1];
  sizes[2] = s[2];
  return 0;
}
extern "C" int ctts_flac_encode_ranges(const int16_t* pcm, const int64_t* counts, const ctts_flac_range* rng_dev, const ctts_flac_range* rng_host,
                                       int32_t n_rng, uint8_t* out, size_t out_bytes, void* work, size_t work_bytes, void* stream) {
  const char* who = "ctts_flac_encode_ranges";
  if (!pcm || !out || !rng_dev || !rng_host || !work) return fail("%s: a null pointer (pcm, out, work and both range tables are needed)", who);
  long long s[5];
  bool wants_counts;
  if (flac_check_table(who, rng_host, n_rng, s, &wants_counts)) return -1;
  if (wants_counts && !counts) return fail("%s: a null pointer (a range has a count_idx, so counts is needed)", who);
  if (((uintptr_t)pcm & 15) || ((uintptr_t)out & 15) || ((uintptr_t)work & 15) || ((uintptr_t)counts & 7))
    return fail("%s: pcm, out and work must be 16-byte aligned, counts 8-byte aligned", who);
  if ((long long)out_bytes < s[1] || out_bytes >= (1ull << 62))
    return fail("%s: out holds %zu bytes, the ranges may need %lld (out of capacity)", who, out_bytes, s[1]);
  if ((long long)work_bytes < s[2] || work_bytes >= (1ull << 62))
    return fail("%s: work holds %zu bytes, %lld are needed (out of capacity)", who, work_bytes, s[2]);
  const uintptr_t p0 = (uintptr_t)pcm, o0 = (uintptr_t)out;
  if (p0 == o0 || (p0 < o0 + (uintptr_t)out_bytes && o0 < p0 + 2 * (uintptr_t)s[4]))
    return fail("%s: out aliases pcm (the encoding is not in place)", who);
  if (s[0] == 0) return 0;                       // nothing but skipped or empty ranges
  CttsDeviceGuard dg(stream);
  long long* meta = (long long*)work;
  CK(launch_flac_encode(pcm, (const long long*)counts, (const FlacRange*)rng_dev, n_rng, s[3], s[0], out, meta,
                        (FlacFrame*)(meta + s[0] + 1 + n_rng), (hipStream_t)stream));
  return 0;
}
static_assert(sizeof(ctts_adpcm_range) == 48 && sizeof(AdpcmRange) == 48 && offsetof(ctts_adpcm_range, block0) == offsetof(AdpcmRange, block0) &&
              offsetof(ctts_adpcm_range, byte0) == offsetof(AdpcmRange, byte0) && offsetof(ctts_adpcm_range, rate) == offsetof(AdpcmRange, rate) &&
              offsetof(ctts_adpcm_range, count_idx) == offsetof(AdpcmRange, count_idx), "ctts_adpcm_range layout");
// the checks of a host table; sizes: the blocks, out bytes, the end of the last range (elements)
static int adpcm_check_table(const char* who, const ctts_adpcm_range* rng_host, int32_t n_rng, long long sizes[3], bool* wants_counts) {
  if (!rng_host) return fail("%s: a null pointer (the host range table is needed)", who);
  if (n_rng < 1 || n_rng > 1024) return fail("%s: need 1 <= n_rng <= 1024 (got %d)", who, n_rng);
  long long end = 0, blocks = 0, bytes = 0;
  *wants_counts = false;
  for (int i = 0; i < n_rng; ++i) {
    const ctts_adpcm_range& r = rng_host[i];
    if (r.rate < 0) return fail("%s: range %d: a rate of %d Hz (0 skips the range; else a positive rate)", who, i, r.rate);
    if (r.start < 0 || (r.start & 7)) return fail("%s: range %d starts at element %lld: starts are multiples of 8", who, i, (long long)r.start);
    if (r.n < 0) return fail("%s: range %d has a negative length (%lld)", who, i, (long long)r.n);
    if (r.start >= (1ll << 46) || r.n >= (1ll << 31)) return fail("%s: range %d lies beyond what a launch can address (n < 2^31)", who, i);
    if (r.start < end) return fail("%s: range %d starts at element %lld, before the end %lld of the ranges in front of it (overlapping or descending)", who,
                                   i, (long long)r.start, end);
    if (r.count_idx < -1 || r.count_idx > 65535) return fail("%s: range %d: count_idx %d is neither -1 nor in 0 .. 65535", who, i, r.count_idx);
    end = r.start + r.n;
    if (r.block0 != blocks) return fail("%s: range %d: block0 is %lld, the ranges in front of it own %lld blocks", who, i, (long long)r.block0, blocks);
    if (r.byte0 != bytes) return fail("%s: range %d: byte0 is %lld, the ranges in front of it own %lld bytes", who, i, (long long)r.byte0, bytes);
    if (r.rate == 0) continue;
    if (r.count_idx >= 0) *wants_counts = true;
    const long long align = 256ll * std::max(1, r.rate / 11025), S = 2 * (align - 4) + 1, nb = (r.n + S - 1) / S;
    blocks += nb;
    bytes += nb * align;
  }
  if (blocks >= (1ll << 31)) return fail("%s: the ranges own %lld blocks, a launch takes fewer than 2^31", who, blocks);
  sizes[0] = blocks;
  sizes[1] = bytes;
  sizes[2] = end;
  return 0;
}
extern "C" int ctts_adpcm_encode_sizes(const ctts_adpcm_range* rng_host, int32_t n_rng, int64_t* sizes) {
  const char* who = "ctts_adpcm_encode_sizes";
  if (!sizes) return fail("%s: a null pointer (sizes[3] is needed)", who);
  long long s[3];
  bool wants_counts;
  if (adpcm_check_table(who, rng_host, n_rng, s, &wants_counts)) return -1;
  sizes[0] = s[0];
  sizes[1] = s[1];
  sizes[2] = (8ll * n_rng + 15) / 16 * 16;
  return 0;
}
extern "C" int ctts_adpcm_encode_ranges(const int16_t* pcm, const int64_t* counts, const ctts_adpcm_range* rng_dev, const ctts_adpcm_range* rng_host,
                                        int32_t n_rng, uint8_t* out, size_t out_bytes, int64_t* used, size_t used_bytes, void* stream) {
  const char* who = "ctts_adpcm_encode_ranges";
  if (!pcm || !out || !rng_dev || !rng_host || !used) return fail("%s: a null pointer (pcm, out, used and both range tables are needed)", who);
  long long s[3];
  bool wants_counts;
  if (adpcm_check_table(who, rng_host, n_rng, s, &wants_counts)) return -1;
  if (wants_counts && !counts) return fail("%s: a null pointer (a range has a count_idx, so counts is needed)", who);
  if (((uintptr_t)pcm & 15) || ((uintptr_t)out & 15) || ((uintptr_t)rng_dev & 7) || ((uintptr_t)used & 7) || ((uintptr_t)counts & 7))
    return fail("%s: pcm and out must be 16-byte aligned, counts, used and the device table 8-byte aligned", who);
  if ((long long)out_bytes < s[1] || out_bytes >= (1ull << 62))
    return fail("%s: out holds %zu bytes, the ranges own %lld (out of capacity)", who, out_bytes, s[1]);
  if (used_bytes < 8 * (size_t)n_rng || used_bytes >= (1ull << 62))
    return fail("%s: used holds %zu bytes, %d are needed (out of capacity)", who, used_bytes, 8 * n_rng);
  const uintptr_t p0 = (uintptr_t)pcm, o0 = (uintptr_t)out;
  if (p0 == o0 || (p0 < o0 + (uintptr_t)out_bytes && o0 < p0 + 2 * (uintptr_t)s[2]))
    return fail("%s: out aliases pcm (the encoding is not in place)", who);
  if (s[0] == 0) return 0;                       // nothing but skipped or empty ranges
  CttsDeviceGuard dg(stream);
  CK(launch_adpcm_encode(pcm, (const long long*)counts, (const AdpcmRange*)rng_dev, n_rng, s[0], out, (long long*)used, (hipStream_t)stream));
  return 0;
}
static_assert(sizeof(ctts_flac_push) == 64 && sizeof(FlacPush) == 64 && offsetof(ctts_flac_push, sample) == offsetof(FlacPush, sample) &&
              offsetof(ctts_flac_push, stage) == offsetof(FlacPush, stage) && offsetof(ctts_flac_push, frame0) == offsetof(FlacPush, frame0) &&
              offsetof(ctts_flac_push, rate) == offsetof(FlacPush, rate) && offsetof(ctts_flac_push, slot) == offsetof(FlacPush, slot) &&
              offsetof(ctts_flac_push, carry) == offsetof(FlacPush, carry) && offsetof(ctts_flac_push, flags) == offsetof(FlacPush, flags) &&
              offsetof(ctts_flac_push, count_idx) == offsetof(FlacPush, count_idx), "ctts_flac_push layout");
// the checks of a host push table; sizes: n_frames, out bytes, work bytes, staging elements, the most slots of one push
static int flac_check_pushes(const char* who, const ctts_flac_push* push_host, int32_t n_push, int32_t n_slots, long long n_pcm,
                             long long sizes[5], bool* wants_counts, bool* wants_mask) {
  if (!push_host) return fail("%s: a null pointer (the host push table is needed)", who);
  if (n_push < 1 || n_push > 1024) return fail("%s: need 1 <= n_push <= 1024 (got %d)", who, n_push);
  if (n_slots < 1) return fail("%s: the state pool has %d slots", who, n_slots);
  if (n_pcm < 0) return fail("%s: n_pcm is negative (%lld)", who, n_pcm);
  long long stage = 0, frames = 0, frames_max = 0, out_bytes = 0;
  *wants_counts = *wants_mask = false;
  for (int i = 0; i < n_push; ++i) {
    const ctts_flac_push& p = push_host[i];
    if (!flac_rate_ok(p.rate))
      return fail("%s: push %d: a rate of %d Hz cannot be coded (a rate of the format's table or 1 .. 65535)", who, i, p.rate);
    if (p.slot < 0 || p.slot >= n_slots) return fail("%s: push %d: slot %d lies outside the pool of %d", who, i, p.slot, n_slots);
    for (int j = 0; j < i; ++j)
      if (push_host[j].slot == p.slot) return fail("%s: pushes %d and %d name slot %d: a stream appears twice in one step", who, j, i, p.slot);
    if (p.start < 0 || (p.start & 7)) return fail("%s: push %d starts at element %lld: starts are multiples of 8", who, i, (long long)p.start);
    if (p.n < 0) return fail("%s: push %d has a negative length (%lld)", who, i, (long long)p.n);
    if (p.n >= (1ll << 31)) return fail("%s: push %d lies beyond what a launch can address (n < 2^31)", who, i);
    if (p.start > n_pcm || p.n > n_pcm - p.start)
      return fail("%s: push %d ends at element %lld, beyond the %lld of pcm", who, i, (long long)(p.start + p.n), n_pcm);
    if (p.carry < 0 || p.carry >= FLAC_MIN_BLOCK) return fail("%s: push %d: a stream carries 0 .. 15 samples (got %d)", who, i, p.carry);
    if (p.flags & ~3) return fail("%s: push %d: unknown flag bits (%d)", who, i, p.flags);
    if (p.count_idx < -1 || p.count_idx > 65535) return fail("%s: push %d: count_idx %d is neither -1 nor in 0 .. 65535", who, i, p.count_idx);
    if (!(p.flags & 1) && p.count_idx >= 0)
      return fail("%s: push %d has a count_idx but is not final (only a stream's last push may leave its length to the device)", who, i);
    if (!(p.flags & 1) && (p.flags & 2))
      return fail("%s: push %d has a keep mask but is not final (only a stream's last push may leave its length to the device)", who, i);
    if (p.sample < 0 || p.sample >= (1ll << 36) || p.sample + p.carry + p.n >= (1ll << 36))
      return fail("%s: push %d would take the stream's sample number to 2^36 (sample %lld, %lld more)", who, i, (long long)p.sample,
                  (long long)(p.carry + p.n));
    if (p.stage != stage) return fail("%s: push %d: stage is %lld, the pushes in front of it own %lld staging elements", who, i, (long long)p.stage, stage);
    if (p.frame0 != frames) return fail("%s: push %d: frame0 is %lld, the pushes in front of it own %lld frame slots", who, i, (long long)p.frame0, frames);
    if (p.count_idx >= 0) *wants_counts = true;
    if (p.flags & 2) *wants_mask = true;
    const long long cap = p.carry + p.n, fr = (cap + FLAC_BLOCK - 1) / FLAC_BLOCK;
    stage += (cap + 7) / 8 * 8;
    frames += fr;
    frames_max = std::max(frames_max, fr);
    out_bytes += 2 * cap + 19 * fr;
  }
  sizes[0] = frames;
  sizes[1] = out_bytes;
  // int64: offsets, total, emitted [n_push] | staged [n_push] | base [n_push]; FlacRange [n_push]; FlacFrame [frames]; the staging buffer
  sizes[2] = ((frames + 1 + 3ll * n_push) * 8 + n_push * (long long)sizeof(FlacRange) + frames * (long long)sizeof(FlacFrame) + 15) / 16 * 16 + 2 * stage;
  sizes[3] = stage;
  sizes[4] = frames_max;
  return 0;
}
extern "C" int ctts_flac_stream_sizes(const ctts_flac_push* push_host, int32_t n_push, int32_t n_slots, int64_t n_pcm, int64_t* sizes) {
  const char* who = "ctts_flac_stream_sizes";
  if (!sizes) return fail("%s: a null pointer (sizes[4] is needed)", who);
  long long s[5];
  bool wants_counts, wants_mask;
  if (flac_check_pushes(who, push_host, n_push, n_slots, n_pcm, s, &wants_counts, &wants_mask)) return -1;
  for (int i = 0; i < 4; ++i) sizes[i] = s[i];
  return 0;
}
extern "C" int ctts_flac_stream_step(const int16_t* pcm, int64_t n_pcm, const uint8_t* mask, const int64_t* counts, const ctts_flac_push* push_dev,
                                     const ctts_flac_push* push_host, int32_t n_push, int16_t* state, int32_t n_slots, uint8_t* out,
                                     size_t out_bytes, void* work, size_t work_bytes, void* stream) {
  const char* who = "ctts_flac_stream_step";
  if (!pcm || !out || !push_dev || !push_host || !work || !state)
    return fail("%s: a null pointer (pcm, out, work, state and both push tables are needed)", who);
  long long s[5];
  bool wants_counts, wants_mask;
  if (flac_check_pushes(who, push_host, n_push, n_slots, n_pcm, s, &wants_counts, &wants_mask)) return -1;
  if (wants_counts && !counts) return fail("%s: a null pointer (a push has a count_idx, so counts is needed)", who);
  if (wants_mask && !mask) return fail("%s: a null pointer (a push has a keep mask, so mask is needed)", who);
  if (((uintptr_t)pcm & 15) || ((uintptr_t)out & 15) || ((uintptr_t)work & 15) || ((uintptr_t)counts & 7) || ((uintptr_t)state & 1))
    return fail("%s: pcm, out and work must be 16-byte aligned, counts 8-byte aligned", who);
  if ((long long)out_bytes < s[1] || out_bytes >= (1ull << 62))
    return fail("%s: out holds %zu bytes, the pushes may need %lld (out of capacity)", who, out_bytes, s[1]);
  if ((long long)work_bytes < s[2] || work_bytes >= (1ull << 62))
    return fail("%s: work holds %zu bytes, %lld are needed (out of capacity)", who, work_bytes, s[2]);
  if (s[0] == 0) return 0;                       // no push holds a sample: nothing is emitted and no slot changes
  CttsDeviceGuard dg(stream);
  long long* meta = (long long*)work;
  long long* staged = meta + s[0] + 1 + n_push;
  long long* base = staged + n_push;
  FlacRange* rng = (FlacRange*)(base + n_push);
  FlacFrame* rec = (FlacFrame*)(rng + n_push);
  int16_t* stage = (int16_t*)((char*)work + s[2] - 2 * s[3]);
  CK(launch_flac_stream(pcm, mask, (const long long*)counts, (const FlacPush*)push_dev, n_push, state, s[4], s[0], out, meta, staged, base,
                        rng, rec, stage, (hipStream_t)stream));
  return 0;
}
static_assert(sizeof(ctts_adpcm_push) == 64 && sizeof(AdpcmPush) == 64 && offsetof(ctts_adpcm_push, stage) == offsetof(AdpcmPush, stage) &&
              offsetof(ctts_adpcm_push, block0) == offsetof(AdpcmPush, block0) && offsetof(ctts_adpcm_push, byte0) == offsetof(AdpcmPush, byte0) &&
              offsetof(ctts_adpcm_push, rate) == offsetof(AdpcmPush, rate) && offsetof(ctts_adpcm_push, slot) == offsetof(AdpcmPush, slot) &&
              offsetof(ctts_adpcm_push, carry) == offsetof(AdpcmPush, carry) && offsetof(ctts_adpcm_push, flags) == offsetof(AdpcmPush, flags) &&
              offsetof(ctts_adpcm_push, count_idx) == offsetof(AdpcmPush, count_idx), "ctts_adpcm_push layout");
// the checks of a host push table; sizes: the blocks, out bytes, work bytes, staging elements, the samples held or pushed
static int adpcm_check_pushes(const char* who, const ctts_adpcm_push* push_host, int32_t n_push, int32_t n_slots, long long n_pcm,
                              long long sizes[5], bool* wants_counts, bool* wants_mask) {
  if (!push_host) return fail("%s: a null pointer (the host push table is needed)", who);
  if (n_push < 1 || n_push > 1024) return fail("%s: need 1 <= n_push <= 1024 (got %d)", who, n_push);
  if (n_slots < 1) return fail("%s: the state pool has %d slots", who, n_slots);
  if (n_pcm < 0) return fail("%s: n_pcm is negative (%lld)", who, n_pcm);
  long long stage = 0, blocks = 0, bytes = 0, samples = 0;
  *wants_counts = *wants_mask = false;
  for (int i = 0; i < n_push; ++i) {
    const ctts_adpcm_push& p = push_host[i];
    if (p.rate < 1) return fail("%s: push %d: a rate of %d Hz (a positive rate)", who, i, p.rate);
    const long long align = 256ll * std::max(1, p.rate / 11025), S = 2 * (align - 4) + 1;
    if (S - 1 > ADPCM_CARRY)
      return fail("%s: push %d: a block at %d Hz holds %lld samples, a stream's slot %d (rates below 55125 Hz)", who, i, p.rate, S, ADPCM_CARRY);
    if (p.slot < 0 || p.slot >= n_slots) return fail("%s: push %d: slot %d lies outside the pool of %d", who, i, p.slot, n_slots);
    for (int j = 0; j < i; ++j)
      if (push_host[j].slot == p.slot) return fail("%s: pushes %d and %d name slot %d: a stream appears twice in one step", who, j, i, p.slot);
    if (p.start < 0 || (p.start & 7)) return fail("%s: push %d starts at element %lld: starts are multiples of 8", who, i, (long long)p.start);
    if (p.n < 0) return fail("%s: push %d has a negative length (%lld)", who, i, (long long)p.n);
    if (p.n >= (1ll << 31)) return fail("%s: push %d lies beyond what a launch can address (n < 2^31)", who, i);
    if (p.start > n_pcm || p.n > n_pcm - p.start)
      return fail("%s: push %d ends at element %lld, beyond the %lld of pcm", who, i, (long long)(p.start + p.n), n_pcm);
    if (p.carry < 0 || p.carry >= S) return fail("%s: push %d: a stream at %d Hz carries 0 .. %lld samples (got %d)", who, i, p.rate, S - 1, p.carry);
    if (p.flags & ~3) return fail("%s: push %d: unknown flag bits (%d)", who, i, p.flags);
    if (p.count_idx < -1 || p.count_idx > 65535) return fail("%s: push %d: count_idx %d is neither -1 nor in 0 .. 65535", who, i, p.count_idx);
    if (!(p.flags & 1) && p.count_idx >= 0)
      return fail("%s: push %d has a count_idx but is not final (only a stream's last push may leave its length to the device)", who, i);
    if (!(p.flags & 1) && (p.flags & 2))
      return fail("%s: push %d has a keep mask but is not final (only a stream's last push may leave its length to the device)", who, i);
    if (p.stage != stage) return fail("%s: push %d: stage is %lld, the pushes in front of it own %lld staging elements", who, i, (long long)p.stage, stage);
    if (p.block0 != blocks) return fail("%s: push %d: block0 is %lld, the pushes in front of it own %lld blocks", who, i, (long long)p.block0, blocks);
    if (p.byte0 != bytes) return fail("%s: push %d: byte0 is %lld, the pushes in front of it own %lld bytes", who, i, (long long)p.byte0, bytes);
    if (p.count_idx >= 0) *wants_counts = true;
    if (p.flags & 2) *wants_mask = true;
    const long long cap = p.carry + p.n, nb = (p.flags & 1) ? (cap + S - 1) / S : cap / S;
    stage += (cap + 7) / 8 * 8;
    blocks += nb;
    bytes += nb * align;
    samples += cap;
  }
  if (blocks >= (1ll << 31)) return fail("%s: the pushes own %lld blocks, a launch takes fewer than 2^31", who, blocks);
  sizes[0] = blocks;
  sizes[1] = bytes;
  // int64: used [n_push] | staged [n_push]; AdpcmRange [n_push]; the staging buffer
  sizes[2] = (16ll * n_push + n_push * (long long)sizeof(AdpcmRange) + 15) / 16 * 16 + 2 * stage;
  sizes[3] = stage;
  sizes[4] = samples;
  return 0;
}
extern "C" int ctts_adpcm_stream_sizes(const ctts_adpcm_push* push_host, int32_t n_push, int32_t n_slots, int64_t n_pcm, int64_t* sizes) {
  const char* who = "ctts_adpcm_stream_sizes";
  if (!sizes) return fail("%s: a null pointer (sizes[4] is needed)", who);
  long long s[5];
  bool wants_counts, wants_mask;
  if (adpcm_check_pushes(who, push_host, n_push, n_slots, n_pcm, s, &wants_counts, &wants_mask)) return -1;
  for (int i = 0; i < 4; ++i) sizes[i] = s[i];
  return 0;
}
extern "C" int ctts_adpcm_stream_step(const int16_t* pcm, int64_t n_pcm, const uint8_t* mask, const int64_t* counts,
                                      const ctts_adpcm_push* push_dev, const ctts_adpcm_push* push_host, int32_t n_push, int16_t* state,
                                      int32_t n_slots, uint8_t* out, size_t out_bytes, void* work, size_t work_bytes, void* stream) {
  const char* who = "ctts_adpcm_stream_step";
  if (!pcm || !out || !push_dev || !push_host || !work || !state)
    return fail("%s: a null pointer (pcm, out, work, state and both push tables are needed)", who);
  long long s[5];
  bool wants_counts, wants_mask;
  if (adpcm_check_pushes(who, push_host, n_push, n_slots, n_pcm, s, &wants_counts, &wants_mask)) return -1;
  if (wants_counts && !counts) return fail("%s: a null pointer (a push has a count_idx, so counts is needed)", who);
  if (wants_mask && !mask) return fail("%s: a null pointer (a push has a keep mask, so mask is needed)", who);
  if (((uintptr_t)pcm & 15) || ((uintptr_t)out & 15) || ((uintptr_t)work & 15) || ((uintptr_t)push_dev & 7) || ((uintptr_t)counts & 7) ||
      ((uintptr_t)state & 1))
    return fail("%s: pcm, out and work must be 16-byte aligned, counts and the device table 8-byte aligned", who);
  if ((long long)out_bytes < s[1] || out_bytes >= (1ull << 62))
    return fail("%s: out holds %zu bytes, the pushes own %lld (out of capacity)", who, out_bytes, s[1]);
  if ((long long)work_bytes < s[2] || work_bytes >= (1ull << 62))
    return fail("%s: work holds %zu bytes, %lld are needed (out of capacity)", who, work_bytes, s[2]);
  const uintptr_t p0 = (uintptr_t)pcm, o0 = (uintptr_t)out;
  if (p0 == o0 || (p0 < o0 + (uintptr_t)out_bytes && o0 < p0 + 2 * (uintptr_t)n_pcm))
    return fail("%s: out aliases pcm (the encoding is not in place)", who);
  if (s[4] == 0) return 0;                       // no push holds or gets a sample: nothing is emitted and no slot changes
  CttsDeviceGuard dg(stream);
  long long* used = (long long*)work;
  long long* staged = used + n_push;
  AdpcmRange* rng = (AdpcmRange*)(staged + n_push);
  int16_t* stage = (int16_t*)((char*)work + s[2] - 2 * s[3]);
  CK(launch_adpcm_stream(pcm, mask, (const long long*)counts, (const AdpcmPush*)push_dev, n_push, state, s[0], out, used, staged, rng, stage,
                         (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_exp_draws(uint64_t seed, int32_t step, int32_t row0, int32_t rows, int32_t V, float* out, void* stream) {
  if (!out || rows <= 0 || V <= 0) return fail("ctts_k_exp_draws: bad arguments");
  CK(launch_exp_draws(seed, step, row0, rows, V, out, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_dwconv_ln(const float* x, const float* w, const float* b, const float* ln_w, const float* ln_b, float eps,
                                int32_t dil, float* y, int32_t B, int32_t F, void* stream) {
  return ctts_k_dwconv_ln_ex(x, w, b, ln_w, ln_b, eps, dil, y, B, F, 512, nullptr, 0, nullptr, stream);
}
extern "C" int ctts_k_dwconv_ln_ex(const float* x, const float* w, const float* b, const float* ln_w, const float* ln_b, float eps,
                                   int32_t dil, float* y, int32_t B, int32_t F, int32_t C, uint16_t* yp, int32_t plane_f16,
                                   const int32_t* seg, void* stream) {
  const hipError_t e = launch_dwconv_ln(x, w, b, ln_w, ln_b, eps, dil, y, B, F, C, (hipStream_t)stream, yp, plane_f16, (const int2*)seg);
  if (e != hipSuccess)
    return fail("ctts_k_dwconv_ln_ex: launch_dwconv_ln refused B %d, F %d, C %d, dil %d, planes %s, seg %s: %s", B, F, C, dil,
                yp ? (plane_f16 ? "fp16" : "bf16 hi/lo") : "none", seg ? "yes" : "no", hipGetErrorString(e));
  return 0;
}
extern "C" int ctts_k_layernorm(const float* x, const float* w, const float* b, float eps, float* y, int32_t rows, void* stream) {
  CK(launch_layernorm(x, w, b, eps, y, rows, 512, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_istft(const float* head, const float* window, const float* twiddle, float* frames, float* wav, int32_t B,
                            int32_t F, void* stream) {
  CK(launch_istft(head, window, twiddle, frames, wav, B, F, (hipStream_t)stream));
  return 0;
}
// the Vocos tail's launchers alone (kernel tests): no checks beyond null pointers -- every bound is the caller's
extern "C" int ctts_k_istft_ragged(const float* head, const float* window, const float* twiddle, float* frames, float* wav,
                                   const int32_t* tok_off, int32_t n_seg, int32_t F_total, int32_t F_max, void* stream) {
  if (!head || !window || !twiddle || !frames || !wav || !tok_off) return fail("ctts_k_istft_ragged: bad arguments");
  CK(launch_istft_ragged(head, window, twiddle, frames, wav, tok_off, n_seg, F_total, F_max, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_gather_windows(const float* hid, int64_t slot_stride, int64_t row_stride, const ctts_window* win, int32_t n_win,
                                     int32_t total_rows, float* packed, int32_t* tok_off, void* stream) {
  if (!hid || !win || !packed || !tok_off) return fail("ctts_k_gather_windows: bad arguments");
  CK(launch_gather_windows(hid, slot_stride, row_stride, (const CodecWindow*)win, n_win, total_rows, packed, tok_off, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_crop_pcm16_windows(const float* wav, const ctts_window* win, int32_t n_win, int32_t out_f32, int32_t product,
                                         float keep_thr, void* out, uint8_t* keep, void* stream) {
  if (!wav || !win || !out) return fail("ctts_k_crop_pcm16_windows: bad arguments");
  CK(launch_crop_pcm16_windows(wav, (const CodecWindow*)win, n_win, out_f32, product, keep_thr, out, keep, (hipStream_t)stream));
  return 0;
}
extern "C" int ctts_k_chunks_pcm16(const float* wav, const float* chunks, const ctts_window* win, const ctts_rs_window* rs, int32_t n_win,
                                   int32_t out_f32, int32_t product, float keep_thr, void* out, uint8_t* keep, void* stream) {
  if (!wav || !chunks || !win || !rs || !out) return fail("ctts_k_chunks_pcm16: bad arguments");
  CK(launch_chunks_pcm16(wav, chunks, (const CodecWindow*)win, (const RsWindow*)rs, n_win, out_f32, product, keep_thr, out, keep,
                         (hipStream_t)stream));
  return 0;
}


// ------------------------------------------------------------------------------------------------
// The one collective of the path: the weights, broadcast from one rank to the others at load -- RCCL over xGMI.
// librccl.so is loaded lazily, on the first call, so a single-GPU host needs neither the library nor a communicator.  The engines hold
// no weight memory of their own (the host allocates every buffer and hands pointers to ctts_*_create), so what is broadcast is the
// host's list of device buffers, in place, BEFORE the engines are created on the receiving ranks.
// ------------------------------------------------------------------------------------------------
namespace {
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, ctts_rccl_id, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool tried = false;
};
Rccl g_rccl;
int rccl_load() {
  if (g_rccl.lib) return 0;
  if (g_rccl.tried) return fail("librccl.so could not be loaded");
  g_rccl.tried = true;
  const char* names[] = {getenv("CTTS_RCCL_LIB"), "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names) {
    if (!n || !*n) continue;
    g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (g_rccl.lib) break;
  }
  if (!g_rccl.lib) return fail("librccl.so not found (dlopen: %s); set CTTS_RCCL_LIB", dlerror());
  g_rccl.GetUniqueId = (int (*)(void*))dlsym(g_rccl.lib, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, ctts_rccl_id, int))dlsym(g_rccl.lib, "ncclCommInitRank");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommDestroy");
  g_rccl.Broadcast = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(g_rccl.lib, "ncclBroadcast");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(g_rccl.lib, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.Broadcast) {
    dlclose(g_rccl.lib); g_rccl.lib = nullptr;
    return fail("librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclBroadcast");
  }
  return 0;
}
int rccl_fail(const char* what, int rc) { return fail("%s: %s (%d)", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error", rc); }
}  // namespace

extern "C" int ctts_rccl_unique_id(ctts_rccl_id* out) {
  if (!out) return fail("ctts_rccl_unique_id: null argument");
  if (rccl_load()) return -1;
  const int rc = g_rccl.GetUniqueId(out);
  return rc == 0 ? 0 : rccl_fail("ncclGetUniqueId", rc);
}
extern "C" int ctts_rccl_comm_create(void** comm, int32_t world, const ctts_rccl_id* id, int32_t rank) {
  if (!comm || !id || world <= 0 || rank < 0 || rank >= world) return fail("ctts_rccl_comm_create: bad arguments");
  if (rccl_load()) return -1;
  const int rc = g_rccl.CommInitRank(comm, world, *id, rank);
  return rc == 0 ? 0 : rccl_fail("ncclCommInitRank", rc);
}
extern "C" void ctts_rccl_comm_destroy(void* comm) {
  if (comm && g_rccl.lib) (void)g_rccl.CommDestroy(comm);
}
extern "C" int ctts_broadcast_weights(void* const* bufs, const size_t* bytes, int32_t n, void* comm, int32_t root, void* stream) {
  if (n < 0 || (n > 0 && (!bufs || !bytes)) || !comm) return fail("ctts_broadcast_weights: bad arguments");
  if (rccl_load()) return -1;
  CttsDeviceGuard dg(stream);
  for (int i = 0; i < n; ++i) {
    if (bytes[i] == 0) continue;
    if (!bufs[i]) return fail("ctts_broadcast_weights: buffer %d is null", i);
    const int rc = g_rccl.Broadcast(bufs[i], bufs[i], bytes[i], /* ncclUint8 */ 1, root, comm, (hipStream_t)stream);   // in place, byte-typed
    if (rc != 0) return rccl_fail("ncclBroadcast", rc);
  }
  return 0;
}
