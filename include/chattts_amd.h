/* chattts_amd -- C ABI of the MI355X-native ChatTTS hot path (libchattts_amd.so).
 *
 * The reference (2noise/ChatTTS) is pure Python and has no FFI for this path; the boundary it
 * offers is the Python call seam that `use_vllm` / `experimental` already use to swap engines
 * (SURVEY.md 8b).  Each entry point below names the reference call it replaces.
 *
 * Conventions
 *   - every pointer named *_dev / documented "device" is a DEVICE pointer owned by the caller (torch
 *     tensors on the host side); the library never allocates or frees device memory, never
 *     synchronises the device, and enqueues everything on the hipStream_t it is given (passed as
 *     void*; NULL = the default stream), so calls are legal inside stream capture;
 *   - return value 0 = ok, negative = error; ctts_last_error() returns a thread-local message;
 *   - a handle is not re-entrant; use one handle per device / per concurrent generate() call.
 */
#ifndef CHATTTS_AMD_H
#define CHATTTS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTTS_F32 0
#define CTTS_BF16 1

typedef struct ctts_gpt ctts_gpt;     /* opaque: GPT engine (weights view + captured decode graph) */
typedef struct ctts_codec ctts_codec; /* opaque: DVAE decoder + Vocos */

const char* ctts_last_error(void);
int ctts_version(void);

/* ------------------------------------------------------------------------------------------------
 * GPT speech-token generator.
 * Replaces `GPT.generate` (ChatTTS/model/gpt.py:316-618): one prefill + N decode steps of
 *   LlamaModel.forward (gpt.py:419-427) -> final-norm hidden capture (:430-436) -> 4 weight-normed heads
 *   (:438-454, embed.py:27-35) -> temperature / repetition penalty / top-p / top-k / EOS mask /
 *   softmax / multinomial (:487-508, processors.py:18-58) -> finish / write-back (:512-577).
 * Weights arrive repacked by the host loader from the reference's safetensors layout:
 *   wqkv[l] = [q_proj; k_proj; v_proj] rows (2304 x 768), wgu[l] = [gate_proj; up_proj] (6144 x 768),
 *   heads = 4 folded weight-norm matrices stacked (2504 x 768, always f32), emb_code = 4 x 626 x 768 f32.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_layers;
  int32_t weight_dtype;            /* CTTS_F32 (parity mode) | CTTS_BF16 (perf mode) for the Llama linears */
  int32_t kv_dtype;                /* dtype of the KV cache */
  int32_t max_pos;                 /* rows of the RoPE tables */
  const void* const* wqkv;         /* host array [n_layers] of device pointers */
  const void* const* wo;           /* [768 x 768] */
  const void* const* wgu;          /* [6144 x 768] */
  const void* const* wd;           /* [768 x 3072] */
  const float* const* ln1;         /* input_layernorm.weight [768] */
  const float* const* ln2;         /* post_attention_layernorm.weight [768] */
  const float* norm;               /* final RMSNorm weight [768] */
  const float* emb_code;           /* [4,626,768] */
  const float* heads;              /* [2504,768] */
  const float* rope_cos;           /* [max_pos,32] float32, built by the host with the reference's own ops */
  const float* rope_sin;
  float rms_eps;
  /* refine-text mode (infer_text=True, gpt.py:406-407,439-440): optional, may be NULL / 0 */
  const float* emb_text;           /* [n_text,768] */
  const float* head_text;          /* [n_text,768] folded weight-norm text head */
  int32_t n_text;                  /* 21178 */
  /* optional (NULL: the decode step uses the row-major kernels): the same four matrices per layer in the fragment-packed order
   * of the weight dtype's decode kernel.  bf16 (csrc/decode.hip): [rows/16][K/32][lane = (k%32)/8*16 + row%16][k%8], one contiguous
   * KiB per (16-row tile, 32-wide k chunk); wqkv with the RoPE row permutation and the folded RMSNorm gain like `wqkv`.
   * f32 (csrc/decode32.hip, needs an f32 KV cache): [rows/16][K/16][lane = (k%16)/4*16 + row%16][k%4] of the plain matrices, wqkv
   * with the RoPE row permutation (no gain folding); same arithmetic, bit for bit, as the row-major f32 kernels. */
  const void* const* wqkv_pk;
  const void* const* wo_pk;
  const void* const* wgu_pk;
  const void* const* wd_pk;
  /* optional (NULL: row-major heads GEMM): `heads` / `head_text` zero-padded to a multiple of 16 rows, in the packed f32 order above
   * ([rows/16][768/16][64][4]); both modes (the heads are always f32); bit-identical logits */
  const float* heads_pk;
  const float* head_text_pk;
  /* optional (NULL: o_proj stays its own launch), perf mode only: o_proj.weight once more, sliced per attention head,
   * [12 heads][8 (k / 8)][768 output columns][8] bf16 = Wo[column][64 head + 8 (k / 8) + (k % 8)].  With it AND the environment
   * variable CTTS_ATT_OPROJ=1 the decode step folds o_proj + residual into the attention launch (csrc/gpt.hip attention_k<OPJ>; HF Llama
   * self_attn.o_proj, examples/onnx/modeling_llama.py:500,557): 83 launches per step instead of 103.  OPT-IN: measured slower than the
   * two launches (profiles/r4b_ab_oproj.log), so by default the pointer is ignored and o_proj stays its own launch. */
  const void* const* wo_hd;
  /* optional (NULL: the f32 MFMA kernels of csrc/decode32.hip), parity mode only, together with the *_pk copies above: the same four
   * matrices as SPLIT-fp16 planes for the decode step (csrc/decode32x.hip; round 5: bf16 planes) -- [2 planes: hi = fp16(w), lo' = fp16((w - hi) * 2^11)]
   * [N/16][K/32][64][8], 22 significant bits, the bf16 fragment order above per plane; wqkv_x3 / wgu_x3 carry the RMSNorm gain of ln1 / ln2 (w' = w * gain[k], folded BEFORE
   * the split) and the q / k row permutation of wqkv_pk.  Three fp16 MFMAs per product (hi*hi, and lo'*hi + hi*lo' on a second accumulator that enters with 2^-11) instead of f32 MFMA at a sixteenth of the rate; the
   * reference's token ids hold on every golden (tests/test_gpu_e2e.py).  The HOST chooses the arithmetic: no planes = exact f32 MFMA; planes =
   * split-fp16 decode steps, certified per call by ctts_gen_state.margin, with ctts_gen_state.proj_exact as the per-call exact fallback. */
  const void* const* wqkv_x3;
  const void* const* wo_x3;
  const void* const* wgu_x3;
  const void* const* wd_x3;
} ctts_gpt_weights;

/* Per-utterance-slot sampling parameters (ctts_gen_state.row_sampling): what the call-wide sampling fields of ctts_gen_state say, for
 * ONE utterance slot, so that requests with different InferCodeParams (core.py:95-110) share one batch / one slot pool -- the role of
 * the reference's per-request SamplingParams in its optional vLLM engine (ChatTTS/model/velocity/sampling_params.py:24).  Code mode
 * only.  128 bytes, every field at a fixed offset (tests/test_sampling_rows_host.py checks the layout against the Python side). */
typedef struct {
  float temperature[4];            /* per-codebook temperature (gpt.py:350-355,487) */
  float pow_table[17];             /* penalty^count, count 0..16, exactly as torch computes it (processors.py:29; rng.penalty_table) */
  int32_t use_penalty;             /* 0: no repetition penalty (penalty == 1, the reference adds no processor, gpt.py:389-391) */
  float top_p_thr;                 /* float32(1 - top_P), rounded on the host (processors.py:38-58, the `cum <= 1 - top_p` test) */
  int32_t use_top_p;               /* 0: top_P is None */
  int32_t top_k;                   /* TopK's k (min_tokens_to_keep 3 is applied by the kernel) */
  int32_t use_top_k;               /* 0: top_K is None */
  int32_t min_new;                 /* min_new_token (gpt.py:494-495) */
  int32_t reserved0;
  uint64_t rng_seed;               /* device generator only: this slot's seed (ctts_gen_state.rng_seed replaced) */
  int32_t rng_per_step;            /* device generator only: 1 = fresh draw every step (manual_seed None; counter word 3 = rng_nonce[b]),
                                      0 = the same draw every step (manual_seed set; counter word 3 = CTTS_RNG_WORD3) */
  int32_t reserved1;
} ctts_sampling_row;

/* One generate() call's device state (every array is caller-allocated, device memory). */
typedef struct {
  int32_t B, T, max_new;           /* rows, padded prompt length, max_new_token (gpt.py:323) */
  int64_t* ids_buf;                /* [B, T+max_new, 4]  inputs_ids_buf (gpt.py:372-379), prompt pre-filled */
  int32_t* len;                    /* [B] tokens present per row; host initialises to T */
  const int32_t* kv_start;         /* [B] number of left-pad slots (attention_mask == 0) */
  uint8_t* finish;                 /* [B] (gpt.py:346) host initialises 0 */
  int32_t* end_idx;                /* [B] (gpt.py:343) host initialises 0 */
  float* hiddens;                  /* [B, max_new, 768] per-step hidden states (gpt.py:435-436) */
  void* kcache;                    /* [n_layers, B, 12, T+max_new, 64] kv_dtype */
  void* vcache;
  const float* q;                  /* [nq, B*4, 626] Exp(1) draws of the CPU generator (gpt.py:501-508) */
  int32_t nq;                      /* 1 when manual_seed is set (same draw every step) */
  const float* temperature;        /* [4] (gpt.py:350-355) */
  const float* pow_table;          /* [17] penalty^f as torch computes it, or NULL (processors.py:29) */
  float top_p_thr;                 /* float32(1 - top_P) */
  int32_t use_top_p;
  int32_t top_k;
  int32_t use_top_k;
  int32_t min_new;                 /* min_new_token (gpt.py:494) */
  int32_t eos;                     /* 625 */
  int32_t row_offset;              /* global index of this shard's row 0 (b*4+k numbering, processors.py:24-27) */
  const int32_t* stop_at;          /* [B] or NULL: benchmark length forcing, not a reference feature */
  void* workspace;                 /* >= ctts_gpt_workspace_bytes(B, T) */
  size_t workspace_bytes;
  const int32_t* row_map;          /* [B] or NULL: compact decode row -> batch slot.  The host packs the utterances that are still
                                      running to the front and refreshes this (and n_active) whenever it polls `finish`; every
                                      array above stays indexed by the batch slot.  NULL = identity / all rows. */
  const int32_t* n_active;         /* device scalar or NULL: number of compact rows the decode step computes.  With row_map == NULL and
                                      n_active != NULL the library compacts ON THE DEVICE: the first kernel of every decode step ranks
                                      the utterances whose finish flag is 0 (ascending slot) and WRITES this scalar (it must be
                                      writable device memory), so finished utterances leave the step at once, without the host. */
  /* Slot-pool (continuous batching) extensions -- all optional, 0 / NULL = the plain generate() layout.  They let a
   * prefill of B freshly admitted utterances write into a larger pool of `kv_batch` utterance slots (row_map[m] = slot
   * of prefill row-group m), with every per-utterance array (ids_buf, len, kv_start, finish, end_idx, hiddens, q,
   * stop_at, prompt_len) allocated for the pool and indexed by slot. */
  int32_t cap;                     /* rows per slot in ids_buf and in the KV cache (0: T + max_new) */
  int32_t hid_cap;                 /* rows per slot in hiddens (0: max_new) */
  int32_t kv_batch;                /* utterance slots in kcache/vcache (0: B) */
  int32_t q_batch;                 /* utterance slots in q (0: B) */
  const int32_t* prompt_len;       /* [slots] padded prompt length of each slot (NULL: T for every row) */
  int32_t infer_text;              /* 1: refine-text mode -- text embedding/head, ONE sampling row per utterance (q is
                                      [nq, B, n_text], temperature[0]), the sampled id is written to all 4 slots
                                      (gpt.py:519-525); repetition penalty must be off */
  const int64_t* teacher_ids;      /* [slots, max_new, 4] or NULL: teacher forcing (evaluation hook, not a reference feature) -- the
                                      token WRITTEN at generation step i of utterance b is teacher_ids[b, i, :] instead of the
                                      sampled one; everything else (finish on EOS, lengths, hidden capture) is unchanged.  Used
                                      to bound the bf16 mode's drift against the reference's golden token stream. */
  int64_t* sampled_ids;            /* [slots, max_new (hid_cap), 4] or NULL: evaluation hook, the companion of teacher_ids -- the token
                                      the sampler itself drew at generation step i (after stop_at forcing, BEFORE teacher forcing
                                      replaced it).  With teacher_ids = the reference's stream this gives the teacher-forced token
                                      agreement rate of a numeric mode (bench.py `bf16_parity`). */
  const int32_t* order;            /* [B] or NULL: visiting order of the device-side compaction (a permutation of the utterance
                                      slots): compact row m of a decode step is the m-th utterance IN THIS ORDER whose finish flag
                                      is 0.  The host passes the utterances by descending context (the contexts of a batch differ
                                      only by the static valid prompt length), so the attention grid starts its longest
                                      (utterance, head) units first.  NULL = ascending slot.  No result depends on it. */
  /* Opt-in DEVICE generator for the Exp(1) draws of the multinomial (both modes; the text mode has ONE sampling row per utterance:
   * global row = row_base[b] or row_offset + b).  The reference draws them from
   * `torch.Generator(device=device)` (gpt.py:39,501-508): on its CPU path that is torch's CPU stream -- the parity contract, served
   * by `q` above -- and on a GPU device its device stream.  With rng_device = 1 `q` is not read: the sampling kernel draws
   * q = -log(u) itself from Philox4x32-10 keyed on rng_seed with counter (token / 4, global sampling row, step), so the default
   * unseeded path needs no per-step host draw / upload.  rng_per_step = 1: a fresh draw every step (manual_seed = None);
   * 0: the same draw every step (manual_seed set -- the reference re-seeds its generator at every step, gpt.py:504-507). */
  int32_t rng_device;
  int32_t rng_per_step;
  const uint64_t* rng_seed;        /* DEVICE scalar (read by the kernel at every step, so a captured graph serves every seed) */
  const uint32_t* rng_nonce;       /* [slots] or NULL, device generator only: a per-utterance-slot word that replaces the constant fourth Philox
                                      counter word.  A slot pool bumps it at every ADMISSION, so successive requests in one slot -- whose step
                                      index restarts at 0 -- do not replay the previous occupant's Exp(1) stream */
  /* PARITY CERTIFICATE (round 6).  [slots] float32 or NULL; the host initialises every entry to +inf.  At every step the sampling kernel
   * lowers margin[b] to the smallest distance -- in units of the TEMPERED logit, logit / temperature -- by which the step's outcome for
   * utterance b was decided: (1) log(r_best / r_second) of the multinomial's argmax(p / q) (gpt.py:497-508); (2) the value gap between the
   * last kept and the first dropped token at the cut the warpers make (processors.py:38-58, TopK / TopP prefix); (3) |log(cum / (1 - top_P))|
   * of the top-p test at the last kept and at the first top-p-dropped rank.  A perturbation of every tempered logit by less than
   * margin / 2 cannot change any sampled token of that utterance: the split-fp16 parity arithmetic (wqkv_x3 ...) is certified per call
   * against its measured logit error bound instead of by sample (chattts_amd/engine.py GptEngine.certify).  NULL: nothing is computed. */
  float* margin;
  /* [B] or NULL: global index of sampling row 0 of utterance b (b_global * 4 in code mode, b_global in text mode) -- replaces
   * row_offset + 4 b (text mode: row_offset + b) when a shard holds a
   * NON-contiguous set of the caller's utterances (length-balanced data-parallel shards, chattts_amd/dist.py; the exact re-run of the
   * utterances a parity certificate flagged).  Keys the rows >= 625 repetition-penalty quirk (processors.py:24-27) and the device
   * generator's counter; `q` stays indexed by the local slot (the host uploads the selected rows of the CPU draw). */
  const int32_t* row_base;
  /* parity mode with BOTH decode copies loaded (wqkv_pk ... and wqkv_x3 ...): 1 = this call's decode steps run the f32 MFMA kernels
   * (csrc/decode32.hip) although the split-fp16 planes are there -- the exact fallback of a certificate that fired.  A captured graph
   * holds the choice it was built with. */
  int32_t proj_exact;
  /* "f32x3" mode, ctts_gpt_prefill only: the number of VALID prompt tokens of the batch (sum of the attention mask = sum of T - kv_start[b]),
   * known to the host.  > 0: the prompt pass runs over those rows only instead of over all B * T left-padded rows (the reference computes
   * the pad rows and never consumes them, gpt.py:234-241).  0: every row.  Same KV cache contents for the valid slots, same token. */
  int32_t prefill_valid_rows;
  /* [slots] or NULL: per-utterance-slot sampling parameters (ctts_sampling_row above).  When set, the sampling of utterance
   * slot b -- decode steps (eager and graph replay), the prefill's step-0 sample, ctts_k_sample -- reads temperature, pow_table,
   * top_p_thr / use_top_p, top_k / use_top_k, min_new, and (device generator) rng_seed / rng_per_step from row_sampling[b] instead of
   * the call-wide fields above, which are then not read (temperature / pow_table / rng_seed may be NULL).  Where the slot's draws come from
   * is unchanged: row_base[b] (or row_offset + 4 b) is its global sampling row (the rows >= 625 penalty quirk, the device generator's
   * counter), q[b] holds its own Exp(1) rows.  The parity certificate (margin) uses the row's own values.  NULL: the call-wide fields.
   * Text mode (infer_text = 1, sample_text_k / ctts_k_sample_text): temperature[0], top_p_thr / use_top_p, top_k / use_top_k, min_new,
   * rng_seed / rng_per_step are read; the mode has no repetition penalty, so use_penalty / pow_table are NOT read there (the host refuses
   * a request that would set them, serving.sampling_row); the global sampling row is row_base[b] (or row_offset + b). */
  const ctts_sampling_row* row_sampling;
} ctts_gen_state;

int ctts_gpt_create(ctts_gpt** out, const ctts_gpt_weights* w);
void ctts_gpt_destroy(ctts_gpt* g);
size_t ctts_gpt_workspace_bytes(int32_t B, int32_t T);

/* step 0 of gpt.py:394: consumes emb[B,T,768] f32 (Embed.forward output, embed.py:52-79), fills the KV
 * cache, writes hiddens[:,0], samples token 0 into ids_buf[:,T], sets len = T+1.  In bf16 mode the four projections of
 * a layer run on LDS-tiled 128x128x64 MFMA tiles when B*T >= 256 rows (csrc/prefill.hip), on the decode kernels below that. */
int ctts_gpt_prefill(ctts_gpt* g, const ctts_gen_state* s, const float* emb, void* stream);
/* The same step 0 in pieces (long prompts, e.g. an `spk_smp` audio-code prompt of hundreds of tokens, core.py:435-453; interleaving
 * the prefill of newly admitted requests with running decode steps): chunk [t0, t0+tc) of the padded prompt of every row, emb_chunk
 * [B, tc, 768] f32.  Chunks must be issued in order; keys of earlier chunks are read from the KV cache.  Only the call with last != 0
 * (t0 + tc == T) runs the final norm / heads / sampling.  The workspace need only hold ctts_gpt_workspace_bytes(B, tc). */
int ctts_gpt_prefill_chunk(ctts_gpt* g, const ctts_gen_state* s, const float* emb_chunk, int32_t t0, int32_t tc, int32_t last, void* stream);
/* one iteration i > 0 of gpt.py:394-577, eager launches */
int ctts_gpt_decode_step(ctts_gpt* g, const ctts_gen_state* s, void* stream);
/* capture one decode step into a hipGraph (all per-step state is read from device memory, so the
 * same executable graph is replayed for every step), then replay it n times */
int ctts_gpt_graph_build(ctts_gpt* g, const ctts_gen_state* s, void* stream);
int ctts_gpt_graph_launch(ctts_gpt* g, int32_t n_steps, void* stream);
/* Round 5: the same captured step for a BOUND on the live rows.  The decode step's grids are sized for the batch B the state describes --
 * 12 attention workgroups and one row of every 16-row projection tile per utterance, finished or not (a finished row's workgroups leave
 * at their first load).  ctts_gpt_graph_build_rows captures the step once more with every grid sized for `rows` < B compact rows; the
 * kernels still read the device-side live count, so ANY bound >= it replays to the same bits as the plain graph.  A host that polls the
 * finish flags anyway (they only ever go up) launches the smallest bound it knows to hold: ctts_gpt_graph_launch_rows(g, n, rows, stream).
 * Needs ctts_gpt_graph_build first; build / destroy of the plain graph drop the bounded ones.  MEASURED: no gain on the C3 bench (the dead
 * workgroups were not what the step waits for, profiles/r5o_ab_graph_rows.log) -- the Python engine uses it only with CTTS_GRAPH_ROWS=1.  No reference counterpart (the reference steps
 * every row until the last one is done, gpt.py:512-518,592). */
int ctts_gpt_graph_build_rows(ctts_gpt* g, const ctts_gen_state* s, int32_t rows, void* stream);
int ctts_gpt_graph_launch_rows(ctts_gpt* g, int32_t n_steps, int32_t rows, void* stream);
void ctts_gpt_graph_destroy(ctts_gpt* g);

/* Per-kernel timing of one launch site (tag) of the eager decode step, for bench.py's roofline leg: the
 * launch goes through hipExtLaunchKernel with start/stop events (dispatch timestamps, as rocprofv3 reads them).
 * tags: 0 embed, 1 qkv, 2 rope_append, 3 attention, 4 o_proj, 5 gate_up, 6 down, 7 final_norm, 8 heads, 9 sample */
int ctts_gpt_profile_begin(ctts_gpt* g, int32_t tag, int32_t max_samples, int32_t stride /* time every stride-th launch */);
/* the individual durations (ms) of the launches timed since profile_begin, in launch order (sample j = the (j * stride)-th launch of the
 * tag); call before profile_end, which resets them.  bench.py fits duration = fixed + bytes / bandwidth over them. */
int ctts_gpt_profile_samples(ctts_gpt* g, float* ms_out, int32_t cap, int32_t* n_samples);
int ctts_gpt_profile_end(ctts_gpt* g, int32_t* n_samples, double* total_ms);

/* ------------------------------------------------------------------------------------------------
 * Acoustic decoder.  Replaces `self.decoder(batch_result)` + `self.vocos.decode(mel)` of
 * Chat._decode_to_wavs / _vocos_decode (ChatTTS/core.py:505-539), i.e. DVAE.forward decode branch
 * (dvae.py:276-297) and vocos.Vocos.decode.  Layout is channels-last: hid [B,T,768] (the per-token
 * hidden states, zero padded), mel [B,2T,100], wav [B,256(2T-1)].
 * Conv weights arrive repacked [Cout][tap][Cin]; depthwise kernels [7][512].
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  /* DVAE decoder (dvae.py:145-161,239) */
  const float* conv_in0_w; const float* conv_in0_b;   /* [128][3][384], [128] */
  const float* conv_in2_w; const float* conv_in2_b;   /* [512][3][128], [512] */
  int32_t n_dvae_blocks;
  const float* const* d_dw_w; const float* const* d_dw_b;    /* [7][512], [512] */
  const float* const* d_ln_w; const float* const* d_ln_b;
  const float* const* d_pw1_w; const float* const* d_pw1_b;  /* [2048][512] */
  const float* const* d_pw2_w; const float* const* d_pw2_b;  /* [512][2048] */
  const float* const* d_gamma;                               /* ConvNeXtBlock.weight [512] */
  const float* conv_out_w;                                   /* [384][512] */
  const float* out_conv_w;                                   /* [100][3][384] */
  const float* coef;                                         /* [100] */
  /* Vocos */
  const float* v_embed_w; const float* v_embed_b;            /* [512][7][100] */
  const float* v_norm_w; const float* v_norm_b;
  int32_t n_vocos_blocks;
  const float* const* v_dw_w; const float* const* v_dw_b;
  const float* const* v_ln_w; const float* const* v_ln_b;
  const float* const* v_pw1_w; const float* const* v_pw1_b;  /* [1536][512] */
  const float* const* v_pw2_w; const float* const* v_pw2_b;  /* [512][1536] */
  const float* const* v_gamma;
  const float* v_final_w; const float* v_final_b;
  const float* head_w; const float* head_b;                  /* [1026][512], [1026] */
  const float* window;                                       /* hann [1024] */
  const float* twiddle;                                      /* [512][2] cos/sin(2 pi k / 1024) */
  /* 0: every dense weight above is float32 [N][K] (f32-input MFMA tiles);
   * 1: every dense weight (conv_in*, *_pw1, *_pw2, conv_out, out_conv, v_embed, head) is instead a packed
   *    split-bf16 tensor [N][Kp/32][2][32] (per row and 32-wide k block: hi values, lo values; Kp = K rounded up to 32, zero padded), consumed by
   *    the bf16x3 tiles (3 bf16 MFMAs per product, f32-class accuracy).  Biases/LN/depthwise stay float32.
   * 2: as 1, but the ConvNeXt point-wise pairs (pwconv1 -> GELU -> pwconv2; 95 % of the decoder's flops) of batches from 12288
   *    frames run on ONE fp16 plane per operand (1 MFMA per product, f32 accumulation, activations saturated to +-65504 where they
   *    are rounded): the waveform stays within 1e-5 RMS of mode 1 (bar: 1e-4), the decoder takes about half the time.  The four
   *    *_x3p arrays below are then REQUIRED and hold fp16 planes [N/32][K/16][lane = (k%16)/8*32 + n%32][k%8]. */
  int32_t gemm_mode;
  /* gemm_mode 1, optional (NULL: the point-wise layers run on the tiles above at every size): the ConvNeXt pwconv1 / pwconv2
   * weights once more as PRE-SPLIT planes in MFMA fragment order, [N/32][K/16][hi|lo][lane = (k%16)/8*32 + n%32][k%8] bf16, for the
   * LDS-DMA staged kernel of csrc/codec_gemm.hip (used from 12288 frames; the depthwise-conv + LayerNorm kernel and the GELU
   * epilogue then write the activations as the same kind of planes) */
  const void* const* d_pw1_x3p; const void* const* d_pw2_x3p;
  const void* const* v_pw1_x3p; const void* const* v_pw2_x3p;
} ctts_codec_weights;

int ctts_codec_create(ctts_codec** out, const ctts_codec_weights* w);
void ctts_codec_destroy(ctts_codec* c);
size_t ctts_codec_workspace_bytes(int32_t B, int32_t F); /* F = mel frames = 2T */
/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: ONE collective, the weight broadcast at load (SURVEY 8b `ctts_broadcast_weights`, 8e; the reference has no data-parallel
 * mode -- ChatTTS/core.py:458-468 batches inside one call only).  One process per GPU; utterances are sharded in contiguous row blocks
 * by the host (chattts_amd/dist.py shard_bounds) and never interact, so nothing else crosses GPUs.  librccl.so is dlopen'ed on the
 * first call (CTTS_RCCL_LIB overrides the name): single-GPU hosts need neither RCCL nor a communicator.  The library owns no weight
 * memory, so the broadcast is over the HOST'S list of device buffers (the repacked weights it is about to hand to ctts_gpt_create /
 * ctts_codec_create), in place, byte-typed, one ncclBroadcast per buffer on `stream` -- pack small tensors into a few flat buffers
 * first: a ring broadcast over xGMI is per-link bound (about 153 GB/s), per-call overhead dominates below ~1 MB.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { char internal[128]; } ctts_rccl_id;   /* = ncclUniqueId: made by ONE rank, carried to the others by the host's own means */
int ctts_rccl_unique_id(ctts_rccl_id* out);
int ctts_rccl_comm_create(void** comm /* ncclComm_t out */, int32_t world, const ctts_rccl_id* id, int32_t rank);   /* ncclCommInitRank on the current device */
void ctts_rccl_comm_destroy(void* comm);
int ctts_broadcast_weights(void* const* bufs, const size_t* bytes, int32_t n, void* comm /* ncclComm_t */, int32_t root, void* stream);

/* float32 waveform -> 16-bit PCM on the device: replaces `float_to_int16` (/root/reference/tools/audio/np.py:7-11) behind Chat.infer --
 * am = 32767 * 32768 // (int(ceil(max |x|)) * 32768); pcm = (x * am) truncated toward zero.  wav: [rows] rows of n samples, ld floats apart;
 * pcm: [rows][n] int16; per_row 0: ONE peak over the whole array (the function applied to a [B, n] block, examples/cmd/stream.py:44),
 * 1: a peak per row (one call per utterance: examples/web/funcs.py:206-209, tools/audio/pcm.py:29); product 0: the float64 product of the
 * reference's numba-jitted runtime, 1: the float32 product plain NumPy >= 2 forms from the same source line; keep_bits: NULL, or
 * [rows][ceil(n / 8)] bytes in np.packbits order, bit = |x| > keep_thr (the mask of Chat.infer's silence strip, core.py:262-265); peak:
 * [rows] uint32 device scratch.  An all-zero input gives zeros (the reference divides by zero).  Stream-ordered, two launches. */
int ctts_float_to_int16(const float* wav, int16_t* pcm, uint8_t* keep_bits, int32_t rows, int64_t n, int64_t ld, int32_t per_row,
                        int32_t product, float keep_thr, uint32_t* peak, void* stream);
/* Shader copy of `bytes` (a multiple of 16; both pointers 16-byte aligned) on `stream`.  `dst` may be PINNED HOST memory (mapped into
 * the device's address space): the float32 waveforms then reach the host -- the `.cpu().numpy()` that ends `Chat._decode_to_wavs`,
 * ChatTTS/core.py:508-510 -- as plain stores over PCIe, without the copy engines. */
int ctts_copy_bytes(void* dst, const void* src, size_t bytes, void* stream);
int ctts_dvae_decode(ctts_codec* c, const float* hid, float* mel, int32_t B, int32_t T, void* workspace, size_t ws_bytes, void* stream);
int ctts_vocos_decode(ctts_codec* c, const float* mel, float* wav, int32_t B, int32_t F, void* workspace, size_t ws_bytes, void* stream);

/* Ragged decode: n_seg utterances of T_i tokens packed back to back along the frame axis, each decoded exactly as if alone (zero padding
 * at its own edges in every convolution; the padded [B, Tmax] entry points above let a short row's tail see the padding's activations).
 *   hid [sum T_i, 768] -> mel [sum F_i, 100] (F_i = 2 T_i) -> wav [sum 256 (F_i - 1)], segment i's samples from 256 (2 tok_off[i] - i).
 * tok_off_dev / tok_off_host: the same n_seg + 1 token offsets (int32, tok_off[0] = 0, strictly ascending -- empty segments are refused),
 * on the device (read by the kernels) and on the host (grid sizes and the checks; the two must agree).  The workspace holds the
 * per-frame segment bounds the kernels read.  Size-dependent kernel choices are keyed on the packed total.  With gemm_mode 0 and fewer
 * than 12288 frames every segment is bit-identical to its B = 1 decode. */
size_t ctts_codec_ragged_workspace_bytes(int32_t n_seg, int32_t total_tokens);   /* 0 when n_seg < 1 or total_tokens < n_seg */
int ctts_dvae_decode_ragged(ctts_codec* c, const float* hid, const int32_t* tok_off_dev, const int32_t* tok_off_host, int32_t n_seg,
                            float* mel, void* workspace, size_t ws_bytes, void* stream);
int ctts_vocos_decode_ragged(ctts_codec* c, const float* mel, const int32_t* tok_off_dev, const int32_t* tok_off_host, int32_t n_seg,
                             float* wav, void* workspace, size_t ws_bytes, void* stream);
/* ctts_float_to_int16 over packed segments (one peak per segment): samples [off[i], off[i+1]) are segment i (int64 offsets, off[0] = 0,
 * strictly ascending, on the device and the host); pcm has the same layout; keep_bits (NULL or sum_i ceil(n_i / 8) bytes) holds segment
 * i's mask from byte sum_{j<i} ceil(n_j / 8) on -- every segment starts on a byte boundary; peak: [n_seg] uint32 device scratch. */
int ctts_float_to_int16_ragged(const float* wav, int16_t* pcm, uint8_t* keep_bits, const int64_t* off_dev, const int64_t* off_host,
                               int32_t n_seg, int32_t product, float keep_thr, uint32_t* peak, void* stream);

/* Grouped strip, convert and compact: the last step of a split_text request (one concatenated waveform, one peak over all its sentences)
 * for many requests in one call.  wav / off as in ctts_float_to_int16_ragged; grp [n_grp + 1] (int32, on the device and the host, the two
 * must agree): segment indices, ascending, grp[0] = 0, grp[n_grp] = n_seg -- segments grp[g] .. grp[g+1]-1 are request g's sentences, in
 * order.  ONE peak and scale per group (`product` as in ctts_float_to_int16).  Group g's kept samples (|x| > keep_thr) are written
 * contiguously, in order, from element gs[g] = sum_{h<g} ceil8(n_h) of pcm (n_h: group h's unstripped sample count) and their number to
 * n_kept[g]; elements behind a group's kept samples are unspecified.  Where every group starts on a multiple of 8 samples -- any decode:
 * a segment holds 256 (2 T - 1) samples -- gs[g] = ceil8(off[grp[g]]) = off[grp[g]], the group's unstripped start; for other offsets
 * ceil8(off[grp[g]]) + n_g could pass ceil8(off[grp[g+1]]), so the padded running sum is the rule.  pcm: sum_g ceil8(n_g) int16, 16-byte
 * aligned.  keep_thr < 0: nothing is stripped -- a plain concatenation under one peak (n_kept[g] = n_g).  An all-zero group converts to
 * zeros.  peak: [n_grp] uint32 device scratch; scratch: ctts_float_to_int16_groups_scratch_bytes(...) bytes of device scratch (per-tile
 * kept counts).  Refused before anything is launched: n_grp < 1, an empty group, a group table that does not run 0 .. n_seg ascending,
 * empty segments / non-ascending offsets, a null peak or count buffer, a group of 2^31 samples or more.  Stream-ordered: a memset and three
 * launches (group peaks + tile counts, a scan per group, convert + scatter); no workgroup waits on another. */
size_t ctts_float_to_int16_groups_scratch_bytes(const int64_t* off_host, int32_t n_seg, const int32_t* grp_host, int32_t n_grp);   /* 0: bad tables */
int ctts_float_to_int16_groups(const float* wav, int16_t* pcm, int64_t* n_kept, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                               const int32_t* grp_dev, const int32_t* grp_host, int32_t n_grp, int32_t product, float keep_thr, uint32_t* peak,
                               void* scratch, size_t scratch_bytes, void* stream);

/* Sample-rate conversion by L/M (new / old rate, reduced) over packed segments: x[off_in[s], off_in[s+1]) -> y[off_out[s], off_out[s+1]),
 * ceil(n_s L / M) samples, every segment as if alone (input outside its own samples reads as zero).  taps: the float32 [L][K] polyphase
 * table on the device, K = 2 width + M:  y[j L + i] = sum_k taps[i][k] x[j M + k - width], one accumulator, k ascending -- a sample does
 * not depend on what it is packed with.  The offsets (int64, first 0, strictly ascending) are given on the device and the host (the two
 * must agree).  sel_dev / sel_host (both NULL: every segment): the n_sel segment indices this call converts -- segments of one pack that
 * go to different rates share off_in / off_out / y, one call per rate.  Refused before anything is launched: L == M, a pair
 * ctts_resample_supported refuses, an empty segment, non-ascending offsets, an output length other than ceil(n L / M), an output of 2^31
 * samples or more.  ctts_resample_supported: 0 = no (a tile's input span or the table is too large), 1 = table read through L2, 2 = table
 * staged in LDS. */
int32_t ctts_resample_supported(int32_t L, int32_t M, int32_t K);
int ctts_resample_ragged(const float* x, const int64_t* off_in_dev, const int64_t* off_in_host, float* y, const int64_t* off_out_dev,
                         const int64_t* off_out_host, int32_t n_seg, const int32_t* sel_dev, const int32_t* sel_host, int32_t n_sel,
                         const float* taps, int32_t L, int32_t M, int32_t K, void* stream);

/* Pitch-preserving time scaling at speed num / den (den = 100, 50 <= num <= 200, num != den) over packed segments: waveform-similarity
 * overlap-add with window N = 1024, synthesis hop HS = 512 and search radius D = 256, x[off_in[s], off_in[s+1]) -> y[off_out[s], off_out[s+1]),
 * n_out = ceil(n_s den / num) samples, every segment as if alone (input outside its own samples reads as zero).  Frame k of
 * F = ceil(n_out / HS) + 1 starts at input sample s_k:  s_0 = -HS;  for k >= 1, a_k = floor(k HS num / den), the template is
 * t[j] = x[s_{k-1} + HS + j], c(d) = sum_{j<N} t[j] x[a_k - HS + d + j] over d in [-D, D), d_k = the d of the largest c (equal c: the
 * smallest |d|, then the negative one), s_k = a_k - HS + d_k.  y[(k-1) HS + j] = window[j + HS] x[s_{k-1} + HS + j] + window[j] x[s_k + j],
 * 0 <= j < HS, each product and the sum rounded to float32.  window: the float32 [N] table 0.5 - 0.5 cos(2 pi j / N) on the device.
 * path: int32 on the device, s_k of segment s at path[path_off[s] + k] -- written by the search, read by the overlap-add, and what a caller
 * needs to reproduce the output.  The three offset tables (int64, first 0, strictly ascending) are given on the device and the host (the
 * two must agree).  The sums run in float32 in a fixed order, so a segment's path and samples do not depend on what it is packed with.
 * Refused before anything is launched: a null pointer, den != 100, num outside 50 .. 200 or num == den, more than 65535 segments, an
 * empty segment, non-ascending offsets, an output length other than ceil(n den / num), a path length other than F, 2^31 samples or more
 * (less the 4096 that a frame may reach past the input: positions are int32).  Stream-ordered: two launches, the search (one workgroup
 * per segment) and the overlap-add. */
int ctts_time_scale_ragged(const float* x, const int64_t* off_in_dev, const int64_t* off_in_host, float* y, const int64_t* off_out_dev,
                           const int64_t* off_out_host, int32_t* path, const int64_t* path_off_dev, const int64_t* path_off_host, int32_t n_seg,
                           const float* window, int32_t num, int32_t den, void* stream);

/* Loudness normalisation: ITU-R BS.1770-4 integrated loudness of packed float32 segments x[off[s], off[s+1]), every segment K-weighted as
 * if alone (two biquads, zero initial state), and y = g32 * x with ONE float32 gain per group of segments; y may be x (otherwise the two
 * do not overlap), both 16-byte aligned.  Segment s is at rate row rate[s] of the coefficient table coef: n_rates rows of 1072 float64
 * that the host computes per rate fs (a multiple of 10 Hz, 8000 .. 48000) -- [0] H = fs / 10, the 100 ms sub-block and the tile;
 * [1] c = ceil(H / 64) | 1, a lane's chunk (odd); [2, 12) b0 b1 b2 a1 a2 of the shelf, then of the high-pass; [16, 32) A^H, row-major, A the 4 x 4
 * state matrix of the cascade in transposed direct form II; [32, 42) the upper triangle of M = sum_{i<H} h_i h_i^T, h_i = C A^i;
 * [48, 1072) A^(l c), l = 0 .. 63.  Sub-block energies e_j (complete sub-blocks only), gating blocks z_i = (e_i + .. + e_{i+3}) / (4 H),
 * l_i = -0.691 + 10 log10 z_i; a segment with fewer than 4 complete sub-blocks is ONE block, its mean square.  Group g is segments
 * grp[g] .. grp[g+1]-1 (the table of the grouped 16-bit conversion): its blocks pass the absolute gate (l_i > -70) and the relative gate
 * (10 LU under the mean of those), L is -0.691 + 10 log10 of the mean of what passed both, its peak is max |x|, and
 * g = min(10^((target[g] - L) / 20), 10^(30 / 20), 10^(-1 / 20) / peak) in float64, rounded once to float32.  No block past the
 * absolute gate: L = -inf and g = 1.  A NaN target: the group is measured, g = 1.  stats: [n_grp] records of 32 bytes on the device --
 * float64 L; float32 peak, g32; int32 blocks, blocks past the absolute gate, blocks past both, the term that bound (0 target, 1 the
 * +30 dB cap, 2 the -1 dBFS ceiling, -1 none).  All float64; the sums run in a fixed order, so a group's record and samples do not depend
 * on what it is packed with.  Every table is given on the device and the host (the two must agree).  Refused before anything is
 * launched: a null pointer, offsets that do not ascend from 0, an empty segment, a pack of 2^31 - 4096 samples or more, more than 65535
 * segments, a rate row outside the table or a row whose H or c is out of range, a group table that does not run 0 .. n_seg ascending,
 * a target outside -40 .. -5, misaligned buffers, scratch under the companion function's size (0: the offsets were refused).
 * Stream-ordered, three launches: the tiles from zero state (one wave each), one workgroup per group (the state chain, the energies'
 * closed-form correction, the gates, the gain), the scale pass. */
size_t ctts_loudness_normalize_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg);
int ctts_loudness_normalize_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                   const int32_t* rate_dev, const int32_t* rate_host, const double* coef_dev, const double* coef_host,
                                   int32_t n_rates, const int32_t* grp_dev, const int32_t* grp_host, int32_t n_grp,
                                   const double* target_dev, const double* target_host, void* stats, void* scratch, size_t scratch_bytes,
                                   void* stream);

/* ctts_loudness_normalize_ragged in front of the peak limiter: the same call and the same refusals, with lim (int32 per group, 0 or 1,
 * on the device and the host) and gain_out (float32 [n_seg] on the device).  A group with lim[g] = 1 gets
 * g = min(10^((target[g] - L) / 20), 10^(30 / 20)) -- the ceiling term is dropped, the limiter enforces it, so its record's bound is 0
 * or 1 -- and its segments are NOT scaled here: they are copied where y is not x and left alone where it is.  Every segment's group
 * gain is written to gain_out, where a ctts_peak_limit_ragged call on the same stream reads it: measurement and limiter are
 * stream-ordered with no host round trip.  A group with lim[g] = 0 is treated as by ctts_loudness_normalize_ragged (in place, a gain
 * of exactly 1 writes nothing).  Scratch: ctts_loudness_normalize_ragged_scratch_bytes. */
int ctts_loudness_limited_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg,
                                 const int32_t* rate_dev, const int32_t* rate_host, const double* coef_dev, const double* coef_host,
                                 int32_t n_rates, const int32_t* grp_dev, const int32_t* grp_host, int32_t n_grp,
                                 const double* target_dev, const double* target_host, const int32_t* lim_dev, const int32_t* lim_host,
                                 float* gain_out, void* stats, void* scratch, size_t scratch_bytes, void* stream);

/* The look-ahead peak limiter (the definition, once, is chattts_amd/limiter.py): packed float32 segments x[off[s], off[s+1]) at rate[s] Hz
 * (a multiple of 10 in 8000 .. 48000; W = rate / 100 samples is 10 ms) with the float32 pre-gain gain[s] (on the device; it may be the
 * gain_out of ctts_loudness_limited_ragged), every segment as if alone: u = gain x; r = 1 where |u| <= T, else T / |u|, with
 * T = float32(C32 (1 - 2^-22)) and C32 = float32(10^(-1 / 20)); m the minimum of r over |k - j| <= W (1 outside the segment); s the mean
 * of m over |j - i| <= W, a float64 sum and division rounded once to float32; y = s u.  So |y| <= C32, a segment with no sample over T
 * comes out as gain x bit for bit, and a NaN passes through.  y may be x (otherwise the two do not overlap), both 16-byte aligned.  The
 * float64 sum is exact, and with it the result independent of the order of summation, while every r >= 2^-19 (gain |x| up to about 4e5).
 * stats: [n_seg] records of 16 bytes on the device -- float32 the pre-gain, min s; int32 the samples with |u| > T, the samples with
 * s < 1.  A segment's samples and record do not depend on what it is packed with.  The offset and rate tables are given on the device
 * and the host (the two must agree).  Refused before anything is launched: a null pointer, offsets that do not ascend from 0, an empty
 * segment, a pack of 2^31 - 4096 samples or more, more than 65535 segments, a rate outside the range or not a multiple of 10,
 * misaligned buffers, y overlapping x in part, scratch under the companion function's size (0: the offsets were refused).
 * Stream-ordered, four launches: the records, the count of samples over T per tile of 2048, the gain curve of the tiles that have
 * such a sample in or next to them (the others leave at once), and y. */
size_t ctts_peak_limit_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg);
int ctts_peak_limit_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg, const int32_t* rate_dev,
                           const int32_t* rate_host, const float* gain_dev, void* stats, void* scratch, size_t scratch_bytes, void* stream);

/* The dynamic range compressor (the definition, once, is chattts_amd/compressor.py): packed float32 segments x[off[s], off[s+1]) at
 * rate[s] Hz (a multiple of 10 in 8000 .. 48000; a block is B = rate / 1000 samples, 1 ms), every segment as if alone.  par holds four
 * int32 per segment: A (attack, 1 .. 20 blocks), H (hold, 0 .. 500 blocks), the index of its gain table (-1: the segment is copied
 * through, its record {1, 0, 0, 0}) and 0.  tab holds n_tab tables of CTTS_CP_TABLE float32, the static curve as data: entry q is the
 * gain at a block peak p with (bits(p) >> 18) - 3296 == q, 32 bins per octave over 2^-24 <= p < 2^8 (below: gain 1; above: the last
 * entry); every entry lies in 2^-18 .. 1.  p the block's peak (a NaN does not count); c its table entry; m the minimum of c over H
 * blocks back and A ahead (1 outside the segment); s the mean of m over blocks b - A .. b, a float64 sum and division rounded once to
 * float32; a[b] = min(s[b-1], s[b]); sample t of block b gets g = a[b] + (a[b+1] - a[b]) (t / B) in float64, each operation rounded once,
 * no fused multiply-add, rounded once more to float32; y = g x.  So g <= 1, a segment with every block under the knee comes back bit for
 * bit, and a NaN passes through.  y may be x (otherwise the two do not overlap), both 16-byte aligned, as is tab_dev.
 * stats: [n_seg] records of 16 bytes on the device (ctts_cp_stats).  A segment's samples and record do not depend on what it is packed
 * with.  Every table is given on the device and the host (the two must agree).  Refused before anything is launched: a null pointer,
 * offsets that do not ascend from 0, an empty segment, a pack of 2^31 - 4096 samples or more, more than 65535 segments, a rate outside
 * the range or not a multiple of 10, A or H out of range, a table index outside -1 .. n_tab - 1, n_tab outside 1 .. n_seg, a table entry
 * outside 2^-18 .. 1, misaligned buffers, y overlapping x in part, scratch under the companion function's size (0: the offsets were
 * refused).  Stream-ordered: a memset of the records, the block peaks and their table entries (one float per block), gain and apply. */
#define CTTS_CP_TABLE 1024
typedef struct {
  float min_gain;         /* the smallest g */
  int32_t n_blocks;       /* blocks with c < 1 */
  int32_t n_touched;      /* samples with g < 1 */
  float peak;             /* the largest block peak */
} ctts_cp_stats;          /* 16 bytes */
size_t ctts_compress_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg);
int ctts_compress_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg, const int32_t* rate_dev,
                         const int32_t* rate_host, const int32_t* par_dev, const int32_t* par_host, const float* tab_dev,
                         const float* tab_host, int32_t n_tab, void* stats, void* scratch, size_t scratch_bytes, void* stream);

/* The output equaliser (the definition, once, is chattts_amd/equalizer.py): packed float32 segments x[off[s], off[s+1]), every segment
 * through a cascade of 1 .. 4 second-order sections as if alone: transposed direct form II in float64 from zero state at the segment's
 * first sample (per section y = b0 x + s0; s0 = b1 x - a1 y + s1; s1 = b2 x - a2 y), the last section's output rounded once to float32.
 * sel holds one int32 per segment: its row of the coefficient table, or -1 (the segment is copied through bit for bit).  coef holds
 * n_rows rows of CTTS_EQ_ROW float64, one per distinct (rate, spec): [0] the number of sections, [1] the rate in Hz (a multiple of 10 in
 * 8000 .. 48000; the kernels do not read it), [2] the chunk (33), [4 + 5 i ..) section i's b0 b1 b2 a1 a2 normalised by a0, [32 + 64 j ..)
 * the state matrix of the cascade to the power 33 * 2^j, j = 0 .. 11, 8 x 8 row-major with zeros beyond two states per section.  The chain
 * is computed in parallel and exactly: chunks of 33 samples run from zero state, the powers carry their end states to the chunks behind
 * them (within a tile of CTTS_EQ_TILE samples by a scan over the chunks, from tile to tile by the same scan over one record per tile),
 * and every chunk runs again from its true entry state.  In float64 that agrees with the serial loop to about 1e-12 of the signal's
 * level: a result differs from the loop's only where it sits on a float32 rounding boundary, by one ulp (an output within about 1e-5
 * of the level of zero has ulps smaller than that error and can be a few of them off).  The tiles are anchored at the segment's first sample: a
 * segment's samples do not depend on what it is packed with.  y may be x (otherwise the two do not overlap), both 16-byte aligned, as
 * are coef_dev and the scratch.  Every table is given on the device and the host (the two must agree).  Refused before anything is
 * launched: a null pointer, offsets that do not ascend from 0, an empty segment, a pack of 2^31 - 4096 samples or more, more than 65535
 * segments, n_rows outside 1 .. n_seg, a row with fewer than 1 or more than 4 sections, with a rate outside the range or not a multiple
 * of 10, with another chunk, with a coefficient or matrix entry that is not finite or a section that is not stable, a row index outside
 * -1 .. n_rows - 1, misaligned buffers, y overlapping x in part, scratch under the companion function's size (0: the offsets were
 * refused).  Stream-ordered, three launches: the tiles' end states, the scan of the tiles per segment, and y (one launch where no segment
 * is longer than a tile). */
#define CTTS_EQ_ROW 800
#define CTTS_EQ_TILE 2112
size_t ctts_equalize_ragged_scratch_bytes(const int64_t* off_host, int32_t n_seg);
int ctts_equalize_ragged(const float* x, float* y, const int64_t* off_dev, const int64_t* off_host, int32_t n_seg, const int32_t* sel_dev,
                         const int32_t* sel_host, const double* coef_dev, const double* coef_host, int32_t n_rows, void* scratch,
                         size_t scratch_bytes, void* stream);

/* The limiter of STREAMS: the segment exists nowhere as a whole, it arrives in pushes, and each step returns the samples the pushes so
 * far decide.  y[i] depends on x[i - 2 W .. i + 2 W], so with pos samples in and more to come, samples [0, pos - 2 W) are out: a stream
 * lags by 2 W samples (20 ms).  One step of one stream: x[in_off, in_off + n_in) are samples [pos, pos + n_in); it writes samples
 * [e_lo, e_lo + n_out) of the limited stream to y[out_off ..], with e_lo = max(0, pos - 2 W) and e_lo + n_out = max(0, pos + n_in - 2 W),
 * or pos + n_in = total on the last push (0: the stream ends empty); positions before sample 0 and from total on are silence.  The chunks of a stream,
 * concatenated, are ctts_peak_limit_ragged of its concatenated pushes bit for bit (under the same condition on the float64 sums), however
 * the signal was cut.  y is a buffer of its own and does not overlap x: nothing is limited in place.
 * carry: [n_slots][2][CTTS_LM_CARRY] float32 on the device, two buffers per slot: a slot keeps its last min(pos, 4 W) RAW samples, a step
 * reads buffer `phase` and writes the other, so the caller flips `phase` after every accepted step of a slot.
 * stats: [n_slots] records of 16 bytes on the device, laid out as ctts_peak_limit_ragged's, accumulated over the samples EMITTED so far
 * by integer atomics (the counts) and an atomic minimum on the bits (min s); after the last push a slot's record is the one-shot record.
 * A slot is fresh by its descriptor alone: at pos == 0 no carry is read, and the records of the descriptors with pos == 0 are reset to
 * {gain, 1, 0, 0} by a launch of its own in front of the step's, so the reset is ordered before the step's atomics by the kernel boundary
 * (nothing has been emitted while pos == 0, so an empty first push resets nothing that counts).
 * One launch over up to 1024 descriptors of any rates and gains; the table is given on the device and the host (the two must agree).  x
 * and y may be null where n_x, n_y is 0.  A step with n_in == 0 or n_out == 0 still moves the carry.  Refused before anything is launched,
 * from the host mirror: a null pointer, n_streams outside 1 .. 1024, a pool without a slot, y overlapping x, a negative length, position
 * or offset, 2^31 samples, a push outside x, a chunk outside y, a rate that is no multiple of 10 Hz in 8000 .. 48000, a gain that is not
 * positive and finite, a total that is neither -1 nor pos + n_in, e_lo, n_out, c_in = min(pos, 4 W) or c_out = min(pos + n_in, 4 W)
 * (0 on the last push) other than these, a phase other than 0 / 1, a slot outside the pool or named twice in the call. */
#define CTTS_LM_CARRY 1920
typedef struct {
  int64_t in_off, n_in;   /* the new samples: x[in_off, in_off + n_in) */
  int64_t pos;            /* samples pushed before them */
  int64_t total;          /* the stream's length when this push is its last, else -1 */
  int64_t e_lo, n_out;    /* the step emits samples [e_lo, e_lo + n_out) of the limited stream */
  int64_t out_off;        /* .. to y[out_off ..] */
  int32_t slot, phase;    /* the state slot; which of its two carry buffers holds samples [pos - c_in, pos) */
  int32_t c_in, c_out;    /* raw samples kept in front of the step; samples [pos + n_in - c_out, pos + n_in) kept behind it (0 on the last push) */
  int32_t rate;           /* Hz */
  float gain;             /* the float32 pre-gain g32 */
} ctts_lm_stream;         /* 80 bytes (limiter stream) */
int ctts_peak_limit_stream_step(const float* x, int64_t n_x, const ctts_lm_stream* st_dev, const ctts_lm_stream* st_host, int32_t n_streams,
                                float* y, int64_t n_y, float* carry, void* stats, int32_t n_slots, void* stream);

/* The compressor of STREAMS (chattts_amd/compressor.py: stream_plan): the segment arrives in pushes.  B = rate / 1000; after a push,
 * `end` = pos + n_in samples are in and end / B blocks are complete.  A step that is not the stream's last emits samples [e_lo, E'),
 * e_lo = max(0, pos / B - A - 1) B and E' = max(0, end / B - A - 1) B: a stream lags by (A + 1) B samples and the open block, whatever the
 * hold; the last step (total == end; 0: the stream ends empty) emits up to the end, and only then the segment's edge rules apply.  The
 * chunks of a stream, end to end, are ctts_compress_ragged of the whole signal bit for bit, however it was cut.  y is a buffer of its own
 * and does not overlap x.  A slot carries, in two halves each (a step reads half `phase` and writes the other: the caller flips `phase`
 * after every accepted step of a slot):
 *   carry: [n_slots][2][CTTS_CP_SCARRY] float32, the raw samples [e_lo, pos): c_in = pos - e_lo, fewer than (A + 2) B;
 *   hold:  [n_slots][2][CTTS_CP_SHIST] float32, the table entries c of the blocks [max(0, e_lo / B - A - H - 1), pos / B): h_in of them, at
 *          most 2 A + H + 2 -- the hold's memory is one float per millisecond, no raw sample older than e_lo is kept.
 * stats: [n_slots] ctts_cp_stats on the device.  A slot's record lives across steps and is touched by order-free atomics only (n_blocks
 * and peak once per block, when its c is computed; min_gain and n_touched over the emitted samples): the CALLER sets it to {1, 0, 0, 0}
 * when it opens the stream, in stream order in front of the first step.  After the last push it is the one-shot record.
 * Each descriptor names its gain table among the n_tab given (device and host; the two must agree).  The c of the blocks a push completes
 * go through `scratch`, from float cb_off: the descriptors' counts of new blocks, end to end; ctts_compress_stream_scratch_bytes(the
 * sum) says how much.  Two launches over up to 1024 descriptors of any rates and specs (one where no push completes a block).  A step
 * with n_in == 0 or n_out == 0 still moves the carry.  Refused before anything is launched, from the host mirror: a null pointer,
 * n_streams outside 1 .. 1024, a pool without a slot, misaligned buffers (x, the tables and the scratch 16 bytes), y overlapping x, a
 * negative length, position or offset, 2^31 samples, a push outside x, a chunk outside y, a rate that is no multiple of 10 Hz in
 * 8000 .. 48000, A outside 1 .. 20, H outside 0 .. 500, a table index outside the n_tab given, n_tab outside 1 .. n_streams, a table entry
 * outside 2^-18 .. 1, a total that is neither -1 nor pos + n_in, e_lo, n_out, c_in, c_out, h_in, h_out or cb_off other than the above (c_out
 * and h_out are 0 on the last push), a phase other than 0 / 1, a slot outside the pool or named twice, a scratch that is too small. */
#define CTTS_CP_SCARRY 1056
#define CTTS_CP_SHIST 544
typedef struct {
  int64_t in_off, n_in;   /* the new samples: x[in_off, in_off + n_in) */
  int64_t pos;            /* samples pushed before them */
  int64_t total;          /* the stream's length when this push is its last, else -1 */
  int64_t e_lo, n_out;    /* the step emits samples [e_lo, e_lo + n_out) of the compressed stream */
  int64_t out_off;        /* .. to y[out_off ..] */
  int64_t cb_off;         /* the c of the blocks this push completes go to the scratch from this float */
  int32_t slot, phase;    /* the state slot; which half of its carry and hold the step reads */
  int32_t rate;           /* Hz */
  int32_t A, H;           /* attack and hold, in blocks */
  int32_t tab;            /* its gain table */
  int32_t c_in, c_out;    /* raw samples kept in front of and behind the step */
  int32_t h_in, h_out;    /* block gains kept in front of and behind the step */
} ctts_cp_stream;         /* 104 bytes (compressor stream) */
size_t ctts_compress_stream_scratch_bytes(int64_t n_blocks);
int ctts_compress_stream_step(const float* x, int64_t n_x, const ctts_cp_stream* st_dev, const ctts_cp_stream* st_host, int32_t n_streams,
                              const float* tab_dev, const float* tab_host, int32_t n_tab, float* y, int64_t n_y, float* carry, float* hold,
                              void* stats, int32_t n_slots, void* scratch, size_t scratch_bytes, void* stream);

/* Pause control: packed float32 segments in[off[s], off[s+1]) lose edge silence and long inner pauses, frame by frame (the definition,
 * once, is chattts_amd/pauses.py).  Segment s has the row rows[8 s ..]: F (samples per 10 ms frame, 80 .. 480), pad, lead, tail, P (frames;
 * P = 0: the segment is copied through), thr (float32 bits, a frame is active when some sample has !(|x| < thr)), the offset of its
 * crossfade table w_in[F] in `fade`, and 0.  fbase[s] is the number of frames in front of segment s (ceil(n / F) frames each).  The kept
 * frames go, in order, to out[off_out[s], off_out[s+1]); off_out (n_seg + 1 int64) and records (8 int32 per segment: frames, active, speech,
 * lead frames removed, tail frames removed, inner runs shortened, inner frames removed, output samples) are written ON THE DEVICE -- the
 * output length depends on the samples.  `out` holds as many samples as `in` (an upper bound) and must not overlap it; both are 16-byte
 * aligned.  A kept sample is a bit-for-bit copy, except one frame per shortened inner run, which is a raised-cosine crossfade
 * (fadd_rn(fmul_rn(w_in[F-1-i], a[i]), fmul_rn(w_in[i], b[i])), no fused multiply-add).  A segment's samples and record do not depend on
 * what it is packed with.  The offset, frame base and row tables are given on the device and the host (the two must agree).  Refused
 * before anything is launched: a null pointer, offsets that do not ascend from 0, an empty segment, a pack of 2^31 - 4096 samples or
 * more, more than 65535 segments, a row out of range, a fade offset outside the table, a frame base table that disagrees with the
 * offsets, misaligned or overlapping buffers, scratch under ctts_trim_pauses_ragged_scratch_bytes(frames, n_seg).  Stream-ordered,
 * four launches: the frames' activity, the plan (one workgroup per segment), the output offsets (one workgroup), the copy. */
size_t ctts_trim_pauses_ragged_scratch_bytes(int64_t frames, int32_t n_seg);
int ctts_trim_pauses_ragged(const float* in, float* out, const int64_t* off_dev, const int64_t* off_host, const int64_t* fbase_dev,
                            const int64_t* fbase_host, const int32_t* rows_dev, const int32_t* rows_host, int32_t n_seg,
                            const float* fade_dev, int32_t n_fade, int64_t* off_out, int32_t* records, void* scratch, size_t scratch_bytes,
                            void* stream);

/* Pause control of STREAMS: a segment arrives in pushes, and the frames ctts_trim_pauses_ragged would keep leave as soon as the rules decide
 * them (chattts_amd/pauses.py: schedule, lags, state).  The chunks of a stream, concatenated, are ctts_trim_pauses_ragged of its concatenated
 * pushes bit for bit, however the signal was cut, and after the last push the slot's record is that call's record (all zero for a stream
 * that ends empty).  One step of one stream: x[in_off, in_off + n_in) are samples [pos, pos + n_in); the chunk is written from y[out_off] on.
 * Its length depends on the samples: res[4 i ..] = (samples written, frames that wait behind the step, copy-list entries, 0) on the device,
 * for the caller to read back in one copy.  y keeps room for `need` F + pos % F + n_in samples from out_off on -- what may wait and what
 * arrives -- and the rooms of a step's streams do not overlap; y does not overlap x.
 * carry: [n_slots][2][CTTS_PA_STREAM_CARRY] float32 on the device, two buffers per slot: the frames that wait (at most `need` =
 * pauses.stream_need of the spec <= CTTS_PA_STREAM_FRAMES, F samples apart) and, at CTTS_PA_STREAM_FRAMES * 480, the pos % F samples of the
 * incomplete frame; a step reads buffer `phase` and writes the other, so the caller flips `phase` after every accepted step of a slot.
 * state: [n_slots][CTTS_PA_STREAM_STATE] int32 on the device, written by the steps only: mode, frames seen, the last active frame, the
 * record (8 int32, pauses.RECORD).  A slot is fresh by its descriptor alone: at pos == 0 neither state nor carry is read.
 * A fixed number of launches (activity of the new frames, a walk of one wave per stream, the copy) over up to 1024 descriptors of any rates
 * and specs; the table is given on the device and the host (the two must agree).  fr_off and list_off are running sums over the
 * descriptors: of nf = (pos % F + n_in) / F new frames (one more for the partial frame of a last push) and of n_list = 2 need + nf + 1
 * entries; scratch holds ctts_trim_pauses_stream_scratch_bytes(sum nf, sum n_list).  Refused before anything is launched, from the host
 * mirror: a null pointer, n_streams outside 1 .. 1024, a pool without a slot, misaligned buffers, y overlapping x, a frame outside 80 .. 480,
 * a spec out of range or needing more than CTTS_PA_STREAM_FRAMES frames, `need`, fr_off, list_off or n_list other than the above, a fade
 * offset outside the table, a negative length, position or offset, 2^31 samples, a push outside x, a room outside y or overlapping
 * another, a phase or last-push flag other than 0 / 1, a slot outside the pool or named twice in the call, scratch too small. */
#define CTTS_PA_STREAM_FRAMES 112
#define CTTS_PA_STREAM_CARRY 54240
#define CTTS_PA_STREAM_STATE 16
#define CTTS_PA_STREAM_RES 4
typedef struct {
  int64_t in_off, n_in;       /* the new samples: x[in_off, in_off + n_in) */
  int64_t pos;                /* samples pushed before them */
  int64_t out_off;            /* the chunk starts at y[out_off] */
  int64_t fr_off;             /* the stream's first new frame among the step's */
  int64_t list_off;           /* the stream's first copy-list entry among the step's */
  int32_t slot, phase;        /* the state slot; which of its two carry buffers the step reads */
  int32_t need;               /* frames the spec can make wait (pauses.stream_need) */
  int32_t fin;                /* 1: the stream's last push */
  int32_t F, pad, lead, tail, P;   /* samples per frame; the spec in frames */
  float thr;                  /* a frame is active when some sample has !(|x| < thr) */
  int32_t fade;               /* the offset of the crossfade table w_in[F] in fade_dev */
  int32_t n_list;             /* copy-list entries kept for the stream */
} ctts_pa_stream;             /* 96 bytes (pause stream) */
size_t ctts_trim_pauses_stream_scratch_bytes(int64_t frames, int64_t entries);
int ctts_trim_pauses_stream_step(const float* x, int64_t n_x, const ctts_pa_stream* st_dev, const ctts_pa_stream* st_host, int32_t n_streams,
                                 float* y, int64_t n_y, float* carry, int32_t* state, int32_t n_slots, const float* fade_dev, int32_t n_fade,
                                 int32_t* res, void* scratch, size_t scratch_bytes, void* stream);

/* Time scaling of streams: the signal of a stream arrives in pushes, its output leaves in chunks, and the concatenation of the chunks (and
 * of the path entries) is ctts_time_scale_ragged's result on the whole signal, bit for bit, however the signal is cut into pushes.
 * With n_avail samples in and more to come, frame k >= 1 may run once need(k) = max(a_{k-1} + D + N - 1, a_k - HS + D + N - 1) <= n_avail;
 * K(n_avail) is the largest such k (0: none).  A push that is not the last runs frames K(pos) < k <= K(pos + n_in) and emits
 * y[HS K(pos), HS K(pos + n_in)) -- possibly nothing; the last one knows total = pos + n_in, runs the frames up to F - 1 and emits the
 * rest up to ceil(total den / num).  After K frames nothing below base(K) = max(0, a_K - HS - D) is read again, so a slot of the state
 * pool keeps x[base(K), n_avail) -- at most CTTS_TS_CARRY floats -- and s_K.
 * carry: [n_slots][2][CTTS_TS_CARRY] float32 on the device, two buffers per slot: a step reads buffer `phase` and writes the other, so the
 * caller flips `phase` after every accepted step of a slot.  state: [n_slots][CTTS_TS_STATE_INTS] int32 on the device.  A slot is fresh
 * by its descriptor alone: at pos == 0 no carry is read, and at k_prev == 0 no state -- a reused slot never sees what it held.
 * The descriptor table is given on the device and the host (the two must agree).  x, y and path may be null where n_x, n_y, n_path is 0.
 * Refused before anything is launched, from the host mirror: a null pointer, n_streams outside 1 .. 1024, den != 100, num outside
 * 50 .. 200 or num == den, a negative length, position or offset, a push outside x, a total that is neither -1 nor pos + n_in,
 * k_prev != K(pos), k_now other than K(pos + n_in) (F - 1 on the last push), n_out other than the plan's or a chunk outside y, path
 * entries outside path, a phase other than 0 / 1, a carry (in front of or behind the step) above CTTS_TS_CARRY, a slot outside the pool
 * or named twice in the call, a position within 4096 of 2^31.  Stream-ordered: one launch, one workgroup per stream. */
#define CTTS_TS_CARRY 2560
#define CTTS_TS_STATE_INTS 4
typedef struct {
  int64_t in_off, n_in;   /* the new samples: x[in_off, in_off + n_in) */
  int64_t pos;            /* their position in the stream */
  int64_t total;          /* the stream's length when this push is the last; -1 otherwise */
  int64_t out_off;        /* first output float in y */
  int64_t path_off;       /* first path entry: k_now - k_prev entries, one more (s_0, in front) when k_prev == 0 < k_now */
  int32_t k_prev, k_now;  /* the step runs frames k_prev < k <= k_now */
  int32_t slot, phase;    /* state slot; which of its two carry buffers holds x[base(k_prev), pos) */
  int32_t num, den;       /* the stream's speed */
  int32_t n_out;          /* samples this step emits */
  int32_t reserved;
} ctts_ts_stream;         /* 80 bytes */
int ctts_time_scale_stream_step(const float* x, int64_t n_x, const ctts_ts_stream* st_dev, const ctts_ts_stream* st_host, int32_t n_streams,
                                float* y, int64_t n_y, int32_t* path, int64_t n_path, float* carry, int32_t* state, int32_t n_slots,
                                const float* window, void* stream);

/* Window decode: the chunks of many streamed utterances that are due at one poll, in ONE ragged pass, each at its own position.
 * hid: a hidden-state store [n_slots][hid_cap][768] float32 (a slot pool's; slot_stride / row_stride in floats, multiples of 4, rows 16-byte
 * aligned).  A window is token rows [t_lo, t_hi) of one slot; it is decoded as one ragged segment -- its edges are sequence edges -- and
 * samples [c_lo, c_hi) of that decode, counted from the window's first sample (sample 512 t_lo of the slot's own decode), are emitted.
 *   out_type 0: float32 (the crop alone); 1: int16, ctts_float_to_int16's arithmetic (`product` as there) with ONE peak per window, taken
 *   over the cropped samples only.
 * out: window i's c_hi - c_lo samples from element out_off[i] = sum_{j<i} ceil8(c_hi_j - c_lo_j) on (every window starts on a multiple of 8
 * samples; the pad samples are zeros), so one copy of sum_i ceil8(n_i) elements delivers every chunk.  keep_bits (may be NULL when no window
 * sets .keep): for a window with .keep != 0 -- a stream's last chunk -- its mask |x| > keep_thr in np.packbits order from byte out_off[i] / 8
 * on (the layout of ctts_float_to_int16_ragged's masks); other windows' bytes are not written.
 * win_dev / win_host: the same n_win entries on the device (read by the kernels) and on the host (sizes and the checks: an empty window, a
 * slot outside the store, t_hi beyond hid_cap, an empty crop or one outside the window's 256 (2 (t_hi - t_lo) - 1) samples are refused before
 * anything is launched).  Stream-ordered on `stream`: one gather launch, the ragged DVAE and Vocos stages, one crop / conversion launch. */
typedef struct {
  int32_t slot;          /* slot of the store */
  int32_t t_lo, t_hi;    /* token rows [t_lo, t_hi) of that slot */
  int32_t c_lo, c_hi;    /* samples to emit, relative to the window's first sample */
  int32_t keep;          /* != 0: also write this window's keep mask */
  int32_t reserved[2];
} ctts_window;           /* 32 bytes */
size_t ctts_codec_windows_workspace_bytes(int32_t n_win, int32_t total_tokens);   /* 0 when n_win < 1 or total_tokens < n_win */
int ctts_codec_decode_windows(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots, int32_t hid_cap,
                              const ctts_window* win_dev, const ctts_window* win_host, int32_t n_win, int32_t out_type, void* out,
                              uint8_t* keep_bits, int32_t product, float keep_thr, void* workspace, size_t ws_bytes, void* stream);

/* Streamed chunks at another sample rate.  A chunk at rate r is outputs [o_lo, o_hi) of the conversion of a whole signal of `total` samples
 * (for a stream: the decode of a token prefix, resampled as one segment alone); those outputs read inputs
 *   [(o_lo / L) M - width, ((o_hi - 1) / L) M + width + M)  clipped to [0, total)            (resample.py, window_inputs)
 * so a WINDOW of the signal that holds them is enough: x[in_off, in_off + n_in) = samples [origin, origin + n_in) of the signal.  Positions
 * outside the window read as zero -- which the checks below make samples outside the signal only, the segment-alone rule.  Given the same
 * samples, a chunk equals outputs [o_lo, o_hi) of ctts_resample_ragged over the whole signal bit for bit (the same accumulation; a tile starts
 * at o_lo, at any phase).  The chunk goes to y[out_off, out_off + o_hi - o_lo), followed by `pad` zeros (0 .. 255).
 * ctts_resample_windows: the kernel alone over packed float windows, all by one L/M.  sel_dev / sel_host (both NULL: every window): the n_sel
 * windows this call converts, so windows of one pack that go to different rates take one call per rate.  n_x / n_y: the floats behind x / y.
 * Refused before anything is launched: a null table, a pair ctts_resample_supported refuses, o_lo < 0, o_hi < o_lo (o_hi == o_lo converts
 * nothing), o_hi beyond ceil(total L / M), a window outside [0, total), a window that does not hold the inputs above, windows outside x or y,
 * more than 1024 windows. */
typedef struct {
  int64_t in_off, n_in;   /* the window's samples in x */
  int64_t origin;         /* position of its first sample in the signal */
  int64_t total;          /* length of the signal */
  int64_t o_lo, o_hi;     /* outputs of the signal's conversion to produce */
  int64_t out_off;        /* first output element */
  int32_t rate;           /* ctts_codec_decode_windows_rate: index into `rates`, < 0: the window stays at 24 kHz; ignored otherwise */
  int32_t pad;            /* zeros written behind the chunk */
} ctts_rs_window;         /* 64 bytes */
int ctts_resample_windows(const float* x, int64_t n_x, const ctts_rs_window* win_dev, const ctts_rs_window* win_host, int32_t n_win, float* y,
                          int64_t n_y, const int32_t* sel_dev, const int32_t* sel_host, int32_t n_sel, const float* taps, int32_t L, int32_t M,
                          int32_t K, void* stream);

/* ctts_codec_decode_windows with one sample rate per window: gather and the ragged DVAE / Vocos stages as there, then the windows that leave
 * 24 kHz are resampled (one launch per distinct rate) into float chunks in the workspace, then ONE conversion launch writes every window's
 * chunk -- the 24 kHz crop, or the resampled chunk -- in ctts_codec_decode_windows's output layout (window i's n_i samples from element
 * sum_{j<i} ceil8(n_j) on, n_i = o_hi - o_lo or c_hi - c_lo; one peak per window over the chunk's own samples; keep masks as there, taken on
 * the chunk's floats).  win: as there; [c_lo, c_hi) of a resampled window is the range the resampler reads.  rs (device and host): entry i
 * describes window i: in_off / n_in = the crop in the packed decode (256 (2 tok_off[i] - i) + c_lo, c_hi - c_lo); rate < 0 and nothing else
 * for a 24 kHz window; else origin = 512 t_lo + c_lo, total = the prefix's 256 (2 Tn - 1) samples, [o_lo, o_hi) non-empty, out_off = the
 * running sum of ceil8(o_hi - o_lo) over the resampled windows before it, pad = the rest to that multiple of 8.  sel (device and host): the
 * resampled windows rate by rate, ascending within a rate.  Refused before anything is launched: everything ctts_codec_decode_windows and
 * ctts_resample_windows refuse (a null table, an unsupported pair, o_hi <= o_lo, a crop that does not hold the inputs the outputs read, more
 * than 1024 windows) and tables that do not agree with each other. */
typedef struct {
  const float* taps;      /* [L][K] float32 on the device */
  int32_t L, M, K, reserved;
} ctts_rate;
size_t ctts_codec_windows_rate_workspace_bytes(int32_t n_win, int32_t total_tokens, int64_t chunk_floats);   /* 0: bad arguments */
int ctts_codec_decode_windows_rate(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots, int32_t hid_cap,
                                   const ctts_window* win_dev, const ctts_window* win_host, const ctts_rs_window* rs_dev,
                                   const ctts_rs_window* rs_host, const int32_t* sel_dev, const int32_t* sel_host, int32_t n_win,
                                   const ctts_rate* rates, int32_t n_rates, int32_t out_type, void* out, uint8_t* keep_bits, int32_t product,
                                   float keep_thr, void* workspace, size_t ws_bytes, void* stream);

/* Window decode of time-scaled streams: crop -> stream step (ctts_time_scale_stream_step's kernel) -> 16-bit conversion around ONE ragged
 * decoder pass.  win: the n_win windows to decode, as in ctts_codec_decode_windows (n_win may be 0: nothing is decoded, streams are only
 * flushed or stepped with empty pushes).  The call emits n_conv chunks in the layout of ctts_codec_decode_windows (chunk e from element
 * sum_{f<e} ceil8(len_f) on, its keep mask when cwin[e].keep -- of cwin only `keep` is read): crs[e].rate < 0: the 24 kHz samples
 * [in_off, in_off + n_in) of the packed decode (window i's first sample is 256 (2 tok_i - i), tok_i the tokens of the windows in front of
 * it); crs[e].rate >= 0: the chunk of stream descriptor ts[rate], with o_lo = 0, o_hi = its n_out (0 allowed: the push made no frame
 * final) and out_off = its out_off: the scaled chunks lie one behind the other in chunk order, each from a multiple of 8 floats on, the path
 * entries likewise (they stay in the workspace).  A descriptor's push x[in_off, in_off + n_in) addresses the packed decode.  The descriptors
 * are sorted into rounds (round_off: n_rounds + 1 ascending indices, host): a stream with several chunks in the call takes them in
 * successive rounds, one launch per round; within a round a slot appears once.  Everything ctts_codec_decode_windows and
 * ctts_time_scale_stream_step refuse is refused here, before any launch.
 * Workspace: ctts_codec_windows_speed_workspace_bytes(n_win, total_tokens, sum ceil8(n_out) + ceil8(path entries)); 0: bad arguments. */
size_t ctts_codec_windows_speed_workspace_bytes(int32_t n_win, int32_t total_tokens, int64_t chunk_floats);
int ctts_codec_decode_windows_speed(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots, int32_t hid_cap,
                                    const ctts_window* win_dev, const ctts_window* win_host, int32_t n_win, const ctts_window* cwin_dev,
                                    const ctts_window* cwin_host, const ctts_rs_window* crs_dev, const ctts_rs_window* crs_host, int32_t n_conv,
                                    const ctts_ts_stream* ts_dev, const ctts_ts_stream* ts_host, const int32_t* round_off, int32_t n_rounds,
                                    float* carry, int32_t* state, int32_t n_ts_slots, const float* ts_window, int32_t out_type, void* out,
                                    uint8_t* keep_bits, int32_t product, float keep_thr, void* workspace, size_t ws_bytes, void* stream);

/* Sample-rate conversion of streams: the signal of a stream arrives in pushes -- it exists nowhere as a whole, like the time scaler's
 * stream -- its conversion leaves in chunks, and the concatenation of the chunks is ctts_resample_ragged's result on the whole signal, bit
 * for bit, however the signal is cut.  Output o = j L + i reads inputs [j M - width, j M + width + M), width = (K - M) / 2.  With
 * P' = pos + n_in samples in and more to come, J(P') = (P' - width - M) / M + 1 frames j are complete (0 while P' < width + M): the step
 * emits outputs [o_lo, E'), o_lo = J(pos) L, E' = J(P') L -- possibly nothing; the last push knows total = P' and emits the rest up to
 * ceil(total L / M), inputs at or beyond total reading as zero.  Afterwards nothing below c' = max(0, (E' / L) M - width) is read again: a
 * slot keeps samples [c', P'), at most K - 1 of them (J > (P' - width - M) / M), within CTTS_RS_CARRY floats.
 * carry: [n_slots][2][CTTS_RS_CARRY] float32 on the device, two buffers per slot: a step reads buffer `phase` and writes the other, so the
 * caller flips `phase` after every accepted step of a slot.  A slot is fresh by its descriptor alone: at pos == 0 no carry is read.
 * One launch over descriptors that share one L/M; the table is given on the device and the host (the two must agree).  x and y may be null
 * where n_x, n_y is 0.  Refused before anything is launched, from the host mirror: a null pointer, a pair ctts_resample_supported refuses,
 * n_streams outside 1 .. 1024, a negative length, position or offset, a pad outside 0 .. 255, 2^31 samples, a push outside x, a total that
 * is neither -1 nor pos + n_in (>= 1), o_lo other than J(pos) L, n_out other than the plan's, a chunk (with its pad) outside y, c_in / c_out
 * other than the plan's or above CTTS_RS_CARRY, a phase other than 0 / 1, a slot outside the pool or named twice in the call. */
#define CTTS_RS_CARRY 512
typedef struct {
  int64_t in_off, n_in;   /* the new samples: x[in_off, in_off + n_in) */
  int64_t pos;            /* samples pushed before them */
  int64_t total;          /* the stream's length when this push is the last; -1 otherwise */
  int64_t o_lo;           /* outputs emitted before this step */
  int64_t n_out;          /* outputs this step emits */
  int64_t out_off;        /* first output float in y */
  int32_t slot, phase;    /* state slot; which of its two carry buffers holds samples [pos - c_in, pos) */
  int32_t c_in, c_out;    /* samples of carry in front of the step; samples [pos + n_in - c_out, pos + n_in) kept behind it (0 on the last push) */
  int32_t pad;            /* zeros written behind the chunk */
  int32_t reserved;
} ctts_rs_stream;         /* 80 bytes */
int ctts_resample_stream_step(const float* x, int64_t n_x, const ctts_rs_stream* st_dev, const ctts_rs_stream* st_host, int32_t n_streams,
                              float* y, int64_t n_y, float* carry, int32_t n_slots, const float* taps, int32_t L, int32_t M, int32_t K,
                              void* stream);

/* ctts_codec_decode_windows_speed with the resampler stage behind the time scaler: a chunk may also be a scaled AND resampled one.
 * Everything up to the time scaler's rounds is as there.  rs_of_ts (host, one entry per time-scale descriptor): -1, or the resampler stream
 * descriptor rs[q] the scaled chunk is pushed into, each named once.  Then rs[q].in_off / n_in = that descriptor's out_off / n_out (the
 * scaled chunk in the workspace), and the output entry of the chunk has o_lo = 0, o_hi = rs[q].n_out, out_off = rs[q].out_off: the resampled
 * chunks lie behind ALL scaled chunks, one behind the other in chunk order, each from a multiple of 8 floats on (pad = the rest to it).
 * The resampler descriptors are sorted into groups (grp_off: n_grp + 1 ascending indices, grp_rate: the group's entry of `rates`; host):
 * one launch per group after the time scaler's rounds, in the order given -- a stream with several chunks in the call takes them in
 * successive groups; within a group a slot appears once.  n_rs = grp_off[n_grp] may be 0 (n_grp 0): the call is
 * ctts_codec_decode_windows_speed.  Everything that call and ctts_resample_stream_step refuse is refused here, before any launch.
 * Workspace: ..._workspace_bytes(n_win, total_tokens, sum ceil8(scaled n_out) + sum ceil8(resampled n_out) + ceil8(path entries)). */
size_t ctts_codec_windows_speed_rate_workspace_bytes(int32_t n_win, int32_t total_tokens, int64_t chunk_floats);
int ctts_codec_decode_windows_speed_rate(ctts_codec* c, const float* hid, int64_t slot_stride, int64_t row_stride, int32_t n_slots,
                                         int32_t hid_cap, const ctts_window* win_dev, const ctts_window* win_host, int32_t n_win,
                                         const ctts_window* cwin_dev, const ctts_window* cwin_host, const ctts_rs_window* crs_dev,
                                         const ctts_rs_window* crs_host, int32_t n_conv, const ctts_ts_stream* ts_dev,
                                         const ctts_ts_stream* ts_host, const int32_t* round_off, int32_t n_rounds, float* carry, int32_t* state,
                                         int32_t n_ts_slots, const float* ts_window, const ctts_rs_stream* rs_dev, const ctts_rs_stream* rs_host,
                                         const int32_t* rs_of_ts, const int32_t* grp_off, const int32_t* grp_rate, int32_t n_grp,
                                         const ctts_rate* rates, int32_t n_rates, float* rs_carry, int32_t n_rs_slots, int32_t out_type,
                                         void* out, uint8_t* keep_bits, int32_t product, float keep_thr, void* workspace, size_t ws_bytes,
                                         void* stream);

/* G.711 companding behind the PCM16 conversion: 16-bit PCM -> one byte per sample, mu-law (law 0) or A-law (law 1), the ITU-T G.191 map
 * (a negative sample is companded from its ones' complement, so G(~x) == G(x) ^ 0x80; chattts_amd/g711.py is the NumPy twin):
 *   mu: a = min((mag >> 2) + 33, 0x1FFF), seg = 1 + bits(a >> 6), code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)), | 0x80 when lin >= 0
 *   A:  ix = mag >> 4; if ix > 15 { e = 1; while ix > 31 { ix >>= 1; e++ }; ix = ix - 16 + (e << 4) }; | 0x80 when lin >= 0; ^ 0x55
 * Range r: elements [start, start + n) of `pcm` become BYTES [start, start + n) of `out` -- element offsets carry over with item size 1, so
 * the offset tables of every PCM16 layout (windows, ragged rows, groups) address the companded output too.  Bytes outside every range, and
 * every byte of a skipped range (law -1), are not written.  One launch (g711_ranges_k) whatever the number of ranges; rng_dev / rng_host:
 * the same table on the device (read by the kernel) and on the host (grid size and the checks).  Refused on the host table before anything
 * is launched: a null pointer, n_rng < 1 or > 1024, a start that is negative or no multiple of 8, a negative n, ranges that overlap or
 * descend, a law outside {-1, 0, 1}, pcm or out not 16-byte aligned, `out` aliasing `pcm`. */
typedef struct {
  int64_t start;          /* first element: of the int16 input and of the uint8 output; a multiple of 8 */
  int64_t n;              /* samples */
  int32_t law;            /* 0 mu-law, 1 A-law, -1 the range is skipped */
  int32_t reserved0;
  int64_t reserved1;
} ctts_g711_range;        /* 32 bytes */
int ctts_g711_encode_ranges(const int16_t* pcm, uint8_t* out, const ctts_g711_range* rng_dev, const ctts_g711_range* rng_host, int32_t n_rng,
                            void* stream);

/* FLAC behind the PCM16 conversion: 16-bit mono PCM -> FLAC frames, losslessly (chattts_amd/flac.py is the NumPy twin, byte for byte).
 * The subset: fixed block size 4096 (frames start FF F8; a shorter last block carries n - 1 in 16 bits), the rate by its table code or in
 * Hz (16 bits), one subframe per frame: CONSTANT when all samples are equal, else FIXED order o in 0 .. min(4, n - 1) with 4-bit Rice
 * parameters k in 0 .. 14 over 2^p partitions, p in 0 .. min(6, ctz(n)), (n >> p) > o, when STRICTLY smaller than VERBATIM.  The choice is
 * exact: the smallest subframe in bits over every (o, p, k per partition), ties to the lowest o, then p, then k -- so a frame is at most
 * 16 + 2 n bytes.  CRC-8 (0x07) over the header, CRC-16 (0x8005) over the frame.
 * Range r: elements [start, start + n) of `pcm` are one signal at `rate` Hz; rate 0: the range is skipped.  count_idx >= 0: the signal's
 * length is min(counts[count_idx], n), read ON THE DEVICE (the kept counts of ctts_float_to_int16_groups; the caller vouches for the
 * index); -1: it is n.  The range owns the frame slots [frame0, frame0 + ceil(n / 4096)), frame0 = the slots of the ranges in front of
 * it (skipped ranges own none).  The frames of all ranges are written back to back from out[0] on, in slot order, so that a range's
 * frames form one slice; bytes behind the total are not written.  `work` receives, from its first byte on, int64 [n_frames + 1] the
 * exclusive byte offset of every slot (an unused slot has length 0) and the total, then int64 [n_rng] each range's signal length: what
 * the host copies before it copies exactly the bytes used.  Three launches (flac_analyse_k, flac_scan_k, flac_pack_k) whatever the
 * number of ranges.  ctts_flac_encode_sizes checks a host table and gives sizes[3] = {n_frames, the bytes `out` must hold
 * (sum of 2 n + 16 ceil(n / 4096)), the bytes `work` must hold}.  Refused on the host table before anything is launched: a null pointer
 * (counts may be null when no range has a count_idx), n_rng < 1 or > 1024, a start that is negative or no multiple of 8, n negative or
 * >= 2^31, ranges that overlap or descend, a rate that is negative or neither in the format's table nor < 65536, a count_idx < -1
 * or > 65535, a frame0 other than the running sum, out_bytes or work_bytes too small, pointers not 16-byte aligned, `out` aliasing `pcm`. */
typedef struct {
  int64_t start;          /* first element of the int16 input; a multiple of 8 */
  int64_t n;              /* samples (with count_idx >= 0: the capacity) */
  int32_t rate;           /* Hz; 0: the range is skipped */
  int32_t count_idx;      /* index into counts, or -1 */
  int64_t frame0;         /* the range's first frame slot */
} ctts_flac_range;        /* 32 bytes */
int ctts_flac_encode_sizes(const ctts_flac_range* rng_host, int32_t n_rng, int64_t* sizes);
int ctts_flac_encode_ranges(const int16_t* pcm, const int64_t* counts, const ctts_flac_range* rng_dev, const ctts_flac_range* rng_host,
                            int32_t n_rng, uint8_t* out, size_t out_bytes, void* work, size_t work_bytes, void* stream);

/* IMA/DVI ADPCM behind the PCM16 conversion: 16-bit mono PCM -> the 4-bit blocks of a WAVE_FORMAT_IMA_ADPCM (0x0011) file
 * (chattts_amd/adpcm.py is the NumPy twin, byte for byte, and states the step and the tables).  align = 256 * max(1, rate / 11025) bytes
 * per block, S = 2 * (align - 4) + 1 samples: bytes 0-1 the block's first sample (little-endian), byte 2 its start index -- the least i
 * with STEP[i] >= |x[1] - x[0]|, 88 when there is none -- byte 3 zero, byte 4 + j the code of sample 1 + 2j in bits 0-3 and of sample
 * 2 + 2j in bits 4-7.  A block's bytes depend on its own samples only; the kernel runs one lane per block.
 * Table-driven: range r says that elements [start, start + n) of `pcm` are one signal at `rate` Hz (0: the range is skipped).  With
 * count_idx >= 0 its length m is min(counts[count_idx], n), read on the device (ctts_float_to_int16_groups' kept counts), else n.  The
 * range owns the blocks [block0, block0 + ceil(n / S)) and the bytes of `out` from byte0 on, both the running sums over the ranges in
 * front of it (skipped ranges own none).  It writes ceil(m / S) whole blocks -- positions at or beyond m read as x[m - 1]; m = 0: none --
 * and nothing else; `used` (int64 [n_rng] on the device) receives m for every range (0 for a skipped one).  One launch
 * (adpcm_encode_k) whatever the number of ranges.  ctts_adpcm_encode_sizes checks a host table and gives sizes[3] = {the blocks, the
 * bytes `out` must hold, the bytes `used` must hold}.  Refused on the host table before anything is launched: a null pointer (counts may
 * be null when no range has a count_idx), n_rng < 1 or > 1024, a start that is negative or no multiple of 8, n negative or >= 2^31,
 * ranges that overlap or descend, a negative rate, a count_idx < -1 or > 65535, a block0 or byte0 that is not the running sum, 2^31
 * blocks or more, pointers that are not 16-byte aligned (counts, used: 8), out or used out of capacity, out aliasing pcm. */
typedef struct {
  int64_t start, n;       /* elements of pcm */
  int64_t block0;         /* the range's first block of the call */
  int64_t byte0;          /* its first byte of out */
  int32_t rate;           /* Hz; 0: the range is skipped */
  int32_t count_idx;      /* index into counts, or -1 */
  int64_t reserved;
} ctts_adpcm_range;       /* 48 bytes */
int ctts_adpcm_encode_sizes(const ctts_adpcm_range* rng_host, int32_t n_rng, int64_t* sizes);
int ctts_adpcm_encode_ranges(const int16_t* pcm, const int64_t* counts, const ctts_adpcm_range* rng_dev, const ctts_adpcm_range* rng_host,
                             int32_t n_rng, uint8_t* out, size_t out_bytes, int64_t* used, size_t used_bytes, void* stream);

/* FLAC for STREAMS: the signal arrives in pushes and leaves as variable-block-size frames (sync FF F9) whose header carries the number of
 * the block's first sample, in up to 36 bits (1 .. 7 bytes).  chattts_amd/flac.py (StreamEncoder) is the NumPy twin, byte for byte; the
 * subframes and their exact search are those above.  The cutting rule: a stream holds `carry` samples (0 .. 15) from its last push in its
 * state slot (`state`: int16 [n_slots][16] on the device); with the push's samples that makes `avail`.  Blocks of 4096 leave from the
 * front; a rest of 16 or more is one more block; a rest of 1 .. 15 stays in the slot -- unless the push is final (flags & 1), which emits
 * it as the stream's last block.  A push with avail < 16 that is not final emits nothing.  So every block but a stream's last has
 * 16 .. 4096 samples, and a frame is at most 19 + 2 n bytes.
 * Push i: elements [start, start + n) of `pcm` continue the stream in `slot`; `sample` is the number of the first staged sample (the
 * first carried one).  A FINAL push may leave its length to the device: count_idx >= 0 takes min(counts[count_idx], n) samples, and
 * flags & 2 keeps only the samples whose bit is set in `mask` (MSB first; the push's bits start at byte start / 8: the keep masks of
 * ctts_codec_decode_windows).  The push owns staging elements [stage, stage + carry + n rounded up to 8) and the frame slots
 * [frame0, frame0 + ceil((carry + n) / 4096)), both the running sums over the pushes in front of it.  The caller keeps carry and sample
 * of every stream (a push that is not final is planned in integers: the rule above) and reads, from the first byte of `work` on, int64
 * [n_frames + 1] the exclusive byte offset of every slot and the total, then int64 [n_push] the samples each push emitted.  The frames of
 * all pushes lie back to back from out[0] on, in slot order.  Four launches (flac_stage_k, flac_analyse_k, flac_scan_k, flac_pack_k)
 * whatever the number of pushes; no launch when no push holds a sample.  ctts_flac_stream_sizes checks a host table and gives sizes[4] =
 * {n_frames, the bytes `out` must hold (sum of 2 (carry + n) + 19 slots), the bytes `work` must hold, the staging elements}.
 * Refused on the host table before anything is launched, all streams left as they were: a null pointer (mask / counts may be null when
 * no push uses them), n_push < 1 or > 1024, a slot outside [0, n_slots) or named twice, a start that is negative or no multiple of 8, a
 * push that ends beyond n_pcm, n negative or >= 2^31, a carry outside 0 .. 15, a rate that is neither in the format's table nor
 * 1 .. 65535, unknown flag bits, a count_idx < -1 or > 65535, a count_idx or a mask on a push that is not final, a negative sample
 * number or one that the push would take to 2^36 (sample + carry + n >= 2^36), a stage or frame0 other than the running sum, out_bytes
 * or work_bytes too small, pointers not 16-byte aligned (counts: 8). */
typedef struct {
  int64_t start;          /* first element of the int16 input; a multiple of 8 */
  int64_t n;              /* samples pushed (with a count_idx or a mask: at most) */
  int64_t sample;         /* the number of the first staged sample */
  int64_t stage;          /* the push's first staging element */
  int64_t frame0;         /* the push's first frame slot */
  int32_t rate;           /* Hz */
  int32_t slot;           /* the stream's state slot */
  int32_t carry;          /* samples the slot holds, 0 .. 15 */
  int32_t flags;          /* 1: final; 2: compact by the keep mask */
  int32_t count_idx;      /* index into counts, or -1 */
  int32_t reserved;
} ctts_flac_push;         /* 64 bytes */
int ctts_flac_stream_sizes(const ctts_flac_push* push_host, int32_t n_push, int32_t n_slots, int64_t n_pcm, int64_t* sizes);
int ctts_flac_stream_step(const int16_t* pcm, int64_t n_pcm, const uint8_t* mask, const int64_t* counts, const ctts_flac_push* push_dev,
                          const ctts_flac_push* push_host, int32_t n_push, int16_t* state, int32_t n_slots, uint8_t* out, size_t out_bytes,
                          void* work, size_t work_bytes, void* stream);

/* IMA ADPCM for STREAMS: the signal arrives in pushes and leaves as the whole blocks of ctts_adpcm_encode_ranges.  A block's bytes depend
 * on its own S = 2 * (align - 4) + 1 samples and the rate only, so the pushes of a stream, concatenated, are the bytes of the one-shot
 * encoder over its samples, however they were cut.  chattts_amd/adpcm.py (StreamEncoder) is the NumPy twin, byte for byte.  The cutting
 * rule: a stream holds `carry` samples (0 .. S - 1) from its earlier pushes in its state slot (`state`: int16 [n_slots][2048] on the
 * device); with the push's samples that makes `avail`.  A push that is not final emits avail / S blocks from the front and leaves
 * avail % S samples in the slot; a final push (flags & 1) emits ceil(avail / S) blocks, the last padded with the last sample, and holds
 * nothing; with avail = 0 it emits nothing.
 * Push i: elements [start, start + n) of `pcm` continue the stream in `slot`.  A FINAL push may leave its length to the device:
 * count_idx >= 0 takes min(counts[count_idx], n) samples, and flags & 2 keeps only the samples whose bit is set in `mask` (MSB first; the
 * push's bits start at byte start / 8: the keep masks of ctts_codec_decode_windows).  The push owns staging elements [stage, stage +
 * carry + n rounded up to 8), the blocks [block0, block0 + nb) of the call and the bytes of `out` from byte0 on (nb * align of them),
 * with nb = (carry + n) / S for a push that is not final and ceil((carry + n) / S) for a final one (an upper bound when its length is
 * left to the device); all three are the running sums over the pushes in front of it.  The caller keeps the carry of every stream (the
 * rule above, in integers) and reads, from the first byte of `work` on, int64 [n_push] the samples each push encoded: nb * S for a push
 * that is not final, everything it held for a final one, which wrote ceil(that / S) blocks.  Two launches (adpcm_stage_k, then
 * adpcm_encode_k over the staging ranges) whatever the number of pushes, one when the pushes own no block, none -- and `work` is left
 * as it was -- when no push holds or gets a sample.  ctts_adpcm_stream_sizes checks a host table and gives sizes[4] = {the blocks (an
 * upper bound), the bytes `out` must hold, the bytes `work` must hold, the staging elements}.
 * Refused on the host table before anything is launched, all streams left as they were: a null pointer (mask / counts may be null when
 * no push uses them), n_push < 1 or > 1024, a slot outside [0, n_slots) or named twice, a start that is negative or no multiple of 8, a
 * push that ends beyond n_pcm, n negative or >= 2^31, a rate below 1 or one whose block does not fit a slot (55125 Hz and above), a
 * carry outside 0 .. S - 1, unknown flag bits, a count_idx < -1 or > 65535, a count_idx or a mask on a push that is not final, a stage,
 * block0 or byte0 other than the running sum, out_bytes or work_bytes too small, pointers not 16-byte aligned (counts: 8), out aliasing
 * pcm. */
typedef struct {
  int64_t start, n;       /* elements of the int16 input; start a multiple of 8 */
  int64_t stage;          /* the push's first staging element */
  int64_t block0, byte0;  /* its first block of the call, its first byte of out */
  int32_t rate, slot, carry, flags;   /* flags 1: final; 2: compact by the keep mask */
  int32_t count_idx, reserved;
} ctts_adpcm_push;        /* 64 bytes */
int ctts_adpcm_stream_sizes(const ctts_adpcm_push* push_host, int32_t n_push, int32_t n_slots, int64_t n_pcm, int64_t* sizes);
int ctts_adpcm_stream_step(const int16_t* pcm, int64_t n_pcm, const uint8_t* mask, const int64_t* counts,
                           const ctts_adpcm_push* push_dev, const ctts_adpcm_push* push_host, int32_t n_push,
                           int16_t* state, int32_t n_slots, uint8_t* out, size_t out_bytes, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Full DVAE (asset/DVAE.safetensors): audio -> 4 x T codes and codes -> mel through the GFSQ codebook.
 * Replaces `self.dvae(wav, "encode")` of `Chat.sample_audio_speaker` (ChatTTS/core.py:179-180 ->
 * DVAE.sample_audio, dvae.py:299-303, encode branch :265-274) and `self.dvae(batch_ids)` of
 * `Chat._decode_to_wavs(result.ids, use_decoder=False)` (core.py:518,535; decode branch dvae.py:276-297
 * with GFSQ._embed :87-97).  Dense weights are float32 [N][K] (f32-input MFMA tiles); convs repacked
 * [Cout][tap][Cin]; depthwise kernels [7][hidden].
 * ---------------------------------------------------------------------------------------------- */
typedef struct ctts_dvae ctts_dvae;

typedef struct {            /* DVAEDecoder(idim, odim, n_layer, bn_dim, hidden)  dvae.py:131-172 */
  int32_t idim, odim, hidden /* 256 | 512 */, bn_dim, n_blocks;
  const float* conv_in0_w; const float* conv_in0_b;   /* [bn][3][idim], [bn] */
  const float* conv_in2_w; const float* conv_in2_b;   /* [hidden][3][bn], [hidden] */
  const float* const* dw_w; const float* const* dw_b;
  const float* const* ln_w; const float* const* ln_b;
  const float* const* pw1_w; const float* const* pw1_b;   /* [4 hidden][hidden] */
  const float* const* pw2_w; const float* const* pw2_b;   /* [hidden][4 hidden] */
  const float* const* gamma;
  const float* conv_out_w;                                 /* [odim][hidden] */
} ctts_trunk_weights;

typedef struct {
  ctts_trunk_weights encoder;   /* 512 -> 1024, hidden 256 (config.py:33-39) */
  ctts_trunk_weights decoder;   /* 512 -> 512,  hidden 256 (config.py:40-46) */
  const float* ds0_w; const float* ds0_b;   /* downsample_conv.0: [512][3][100] */
  const float* ds1_w; const float* ds1_b;   /* downsample_conv.2 (k4, stride 2, pad 1) repacked as a k3 conv over frame
                                             * pairs: [512][3][1024] = {[0, W0], [W1, W2], [W3, 0]} */
  const float* out_conv_w;                  /* [100][3][512] */
  const float* coef;                        /* [100] */
  /* GroupedResidualFSQ(dim 1024, levels, num_quantizers R, groups G): per group project_in / project_out */
  const float* q_in_w; const float* q_in_b;     /* [G][4][D], [G][4] */
  const float* q_out_w; const float* q_out_b;   /* [G][D][4], [G][D] */
  int32_t levels[4];
  int32_t G, R, D;                          /* 2, 2, 512 */
  int32_t bound_first;                      /* 1: residual loop starts from bound(project_in(x)) (current library) */
  /* MelSpectrogram(n_fft 1024, hop 256, n_mels 100, center, power 1) buffers */
  const float* mel_window;                  /* [1024] */
  const float* mel_fb;                      /* [100][516]: fb^T, K padded 513 -> 516 with zeros */
  const float* twiddle;                     /* [512][2] cos/sin(2 pi k / 1024) */
} ctts_dvae_weights;

int ctts_dvae_create(ctts_dvae** out, const ctts_dvae_weights* w);
void ctts_dvae_destroy(ctts_dvae* c);
int32_t ctts_dvae_code_frames(int32_t n_samples);            /* T for a clip: F = 1 + n/256 mel frames, T = (F-2)/2 + 1 */
size_t ctts_dvae_encode_workspace_bytes(int32_t n_samples);
size_t ctts_dvae_decode_workspace_bytes(int32_t B, int32_t T);
/* wav [n_samples] f32 (24 kHz) -> codes [T][4] int32 (row t = the 4 code slots of frame t; DVAE.sample_audio
 * returns the transpose [4][T]) */
int ctts_dvae_encode(ctts_dvae* c, const float* wav, int32_t n_samples, int32_t* codes, void* workspace, size_t ws_bytes, void* stream);
/* codes [B][T][4] int64 (zero padded rows, core.py:525-533) -> mel [B][2T][100] */
int ctts_dvae_decode_codes(ctts_dvae* c, const int64_t* codes, float* mel, int32_t B, int32_t T, void* workspace, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Single-kernel entry points (unit parity tests call the kernels through these).
 * ---------------------------------------------------------------------------------------------- */
int ctts_k_gemm(int32_t tiled /* 0 skinny, 1 f32 tiles, 2 split-bf16 tiles */, const float* A, const void* W, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldc,
                int32_t wt, int32_t epi, const float* norm_w, float eps, const float* res, int32_t ldr, const float* bias,
                const float* gamma, int32_t taps, int32_t cin, int32_t frames, int32_t pad, int32_t dil, void* stream);
/* split-bf16 GEMM on pre-split planes in MFMA fragment order (csrc/codec_gemm.hip): Ap / Wp / Cp are
 * [rows/32][K/16][hi|lo][64][8] bf16 with rows padded to 256; epi 0: Cp = planes of gelu(A W^T + bias) (a [rows][N] matrix),
 * epi 1: C = res + gamma * (A W^T + bias), f32 [M][N].  N % 256 == 0, K % 32 == 0. */
int ctts_k_gemm_x3p(const uint16_t* Ap, const uint16_t* Wp, int32_t M, int32_t N, int32_t K, int32_t epi, const float* bias,
                    const float* gamma, const float* res, float* C, uint16_t* Cp, void* stream);
/* the same on ONE fp16 plane per operand (gemm_mode 2): Ap / Wp / Cp are [rows/32][K/16][64][8] fp16; K % 64 == 0 */
int ctts_k_gemm_h1p(const uint16_t* Ap, const uint16_t* Wp, int32_t M, int32_t N, int32_t K, int32_t epi, const float* bias,
                    const float* gamma, const float* res, float* C, uint16_t* Cp, void* stream);
/* a HIP stream confined to n_cus compute units (first_cu, first_cu + stride, ...): hipExtStreamCreateWithCUMask.  The host runs the acoustic
 * decoder of one batch on such a stream while the next batch is generated on the others (the overlapped DVAE / ISTFT side stream of BASELINE
 * config 4, at batch level: CodecEngine.decode_to_wavs_async); destroy with ctts_stream_destroy */
int ctts_stream_create_cu_mask(int32_t first_cu, int32_t n_cus, int32_t stride, int32_t complement /* 1: every CU but those */, void** stream);
int ctts_stream_destroy(void* stream);
/* one ConvNeXt MLP in ONE launch: C = C + gamma * (GELU(A W1^T + b1) W2^T + b2), A [M][512] / W1 [inter][512] / W2 [512][inter] as
 * fp16 planes (planes = 1), C [M][512] f32 in place; bit-identical to ctts_k_gemm_h1p(epi 0) followed by ctts_k_gemm_h1p(epi 1)
 * (ConvNeXtBlock.pwconv1 -> act -> pwconv2 -> gamma -> residual, ChatTTS/model/dvae.py:46-66) */
int ctts_k_mlp_fused(const uint16_t* Ap, const uint16_t* W1p, const uint16_t* W2p, int32_t M, int32_t inter, const float* b1,
                     const float* b2, const float* gamma, float* C, int32_t planes, void* stream);
/* perf-mode projection: bf16 activations/weights, optional per-row 1/rms from 48 partial sums of squares,
 * epi 0 = f32 store, 1 = residual add (+ bf16 copy + new partial sums), 2 = SiLU(gate)*up -> bf16 */
int ctts_k_gemm_fast(const uint16_t* A, int32_t lda, const uint16_t* W, int32_t M, int32_t N, int32_t K, const float* ssq_in, float eps,
                     int32_t epi, float* C32, int32_t ldc, uint16_t* Cb, int32_t ldcb, float* ssq_out, void* stream);
/* perf-mode fused RMSNorm-scale + QKV + RoPE + KV append (W rows permuted as engine.py `rope_row_perm` does) */
int ctts_k_qkv_rope(const uint16_t* A, const uint16_t* W, int32_t M, const float* ssq_in, float eps, float* qkv, uint16_t* kcache,
                    uint16_t* vcache, int32_t cmax, const float* cos_tab, const float* sin_tab, int32_t q_per_b, const int32_t* len,
                    const int32_t* kv_start, int32_t force_mb, void* stream);
/* the same as the prompt pass launches it: row m of a q_per_b > 1 launch appends at KV slot slot0 + m % q_per_b of utterance
 * row_map[m / q_per_b] (row_map NULL: m / q_per_b) -- a later chunk of a prompt, a row group admitted into a slot pool; kv_start is indexed
 * by the utterance.  Refuses null pointers and a chunk that does not fit the cmax cache rows. */
int ctts_k_qkv_rope_ex(const uint16_t* A, const uint16_t* W, int32_t M, const float* ssq_in, float eps, float* qkv, uint16_t* kcache,
                       uint16_t* vcache, int32_t cmax, const float* cos_tab, const float* sin_tab, int32_t q_per_b, const int32_t* len,
                       const int32_t* kv_start, int32_t slot0, const int32_t* row_map, int32_t force_mb, void* stream);
/* decode-step projection on fragment-packed operands (csrc/decode.hip): Ap [ceil(M/16)][K/32][64][8] bf16, Wp packed likewise
 * (epi 2: gate tiles then up tiles); epi 1 = residual add (C32 in place, Cp packed bf16 copy with kch_out = N/32, ssq_out),
 * 2 = SiLU(gate)*up -> Cp packed (kch_out = N/32).  n_active: device scalar or NULL.  force_mb: rows/16 per workgroup (0 = default) */
int ctts_k_gemm_dec(const uint16_t* Ap, const uint16_t* Wp, int32_t M, int32_t N, int32_t K, const int32_t* n_active, const float* ssq_in,
                    float eps, int32_t epi, float* C32, int32_t ldc, uint16_t* Cp, int32_t kch_out, float* ssq_out, int32_t force_mb,
                    void* stream);
/* the same for the f32 parity mode (csrc/decode32.hip): Ap [ceil(M/16)][K/16][64][4] f32, Wp packed likewise; norm_w != NULL: RMSNorm
 * prologue (X = the same rows row-major, ldx) ; epi 0 = store C row-major, 1 = C = res + acc (row-major) and Cp (packed, kch_out = N/16),
 * 2 = SiLU(gate)*up -> Cp.  Bit-identical to ctts_k_gemm(tiled = 0, wt = f32) on the same values. */
int ctts_k_gemm_dec32(const float* Ap, const float* Wp, int32_t M, int32_t N, int32_t K, const int32_t* n_active, const float* X, int32_t ldx,
                      const float* norm_w, float eps, int32_t epi, float* C, int32_t ldc, const float* res, int32_t ldr, float* Cp,
                      int32_t kch_out, int32_t force_mb, int32_t n_cols /* epi 0: columns of C that exist (N padded to 16), 0 = N */,
                      void* stream);
/* The same projections on SPLIT-bf16 operands (csrc/decode32x.hip; ctts_gpt_weights.wqkv_x3 ...): Ap / Wp = hi planes in the bf16 fragment order
 * ([rows/16][K/32][64][8]), the lo planes a_plane / w_plane ELEMENTS behind them; three bf16 MFMAs per product (lo*hi + hi*lo + hi*hi), f32
 * accumulation.  X != NULL (K = 768): RMSNorm launch -- 1 / rms of the rows of X (row-major f32, gemm_skinny_k's arithmetic) scales the
 * accumulator, the gain is expected folded into W; ssq_in != NULL instead: [rows][48] partial sums of squares of the rows (one per 16 columns, what
 * the decode step's producers leave); ssq_out (epi 1): the same partials of the NEW rows.  force_mb: 0 = the launcher's choice, else rows per
 * workgroup / 16 (1 | 2 | 4), + 8 for eight instead of four waves.  epi 1 = C = res + acc (row-major f32), Cp = its planes (c_plane elements apart, kch_out =
 * N / 32) and optionally Cp32 = its packed f32 copy; epi 2 = SiLU(gate) * up -> Cp planes (W = gate tiles then up tiles).  Reference ops:
 * examples/onnx/modeling_llama.py:293,415-417,500. */
int ctts_k_gemm_dec32x(const uint16_t* Ap, int64_t a_plane, const uint16_t* Wp, int64_t w_plane, int32_t M, int32_t N, int32_t K,
                       const int32_t* n_active, const float* X, int32_t ldx, float eps, int32_t epi, float* C, int32_t ldc, const float* res,
                       int32_t ldr, uint16_t* Cp, int64_t c_plane, int32_t kch_out, float* Cp32, int32_t force_mb, const float* ssq_in,
                       float* ssq_out, void* stream);
/* Round 6: the LDS-tiled split-bf16 GEMM of the "f32x3" mode's PROMPT pass (csrc/prefill32x.hip): C = epi(rstd[row] * ((A diag(norm_w)) W^T)),
 * A [M, lda] and W [N (2N for epi 2: gate rows then up rows), K] float32 row-major, split hi | lo by the tile loader, three bf16 MFMAs per
 * product, f32 accumulation.  epi 0 = store, 1 = C = res + acc, 2 = silu(gate) * up.  norm_w / rstd: both or neither.  K % 32 == 0,
 * N % 128 == 0 (epi 2: % 64).  Reference ops: HF Llama projections, examples/onnx/modeling_llama.py:259-295,455-505. */
int ctts_k_gemm_pre_x3(const float* A, int32_t lda, const float* W, float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi,
                       const float* norm_w, const float* rstd, const float* res, int32_t ldr, void* stream);
/* which decode32 kernel the calling thread's last ctts_k_gemm_dec32 / decode step picked: "rms16" | "m16" | "generic" (all bit-identical), or "fnorm16"
 * (the fused final norm + heads launch) */
const char* ctts_k_dec32_last_variant(void);
int ctts_k_rows_prep(const float* x32, uint16_t* xb, float* ssq, int32_t M, void* stream);
int ctts_k_rope_append(float* qkv, void* kcache, void* vcache, int32_t kv_dtype, int32_t cmax, const float* cos_tab, const float* sin_tab,
                       int32_t q_per_b, const int32_t* len, const int32_t* kv_start, int32_t M, void* stream);
int ctts_k_attention(const float* qkv, const void* kcache, const void* vcache, int32_t kv_dtype, int32_t cmax, float* out,
                     int32_t q_per_b, const int32_t* len, const int32_t* kv_start, int32_t M, void* stream);
/* prefill attention of the perf mode over a bf16 KV cache: M = B * q_per_b query rows (row m: utterance m / q_per_b, KV slot
 * slot0 + m % q_per_b -- slot0 > 0: a later chunk of a prompt prefilled in pieces), f32 output [M,768]; from q_per_b >= 128 the
 * flash-style MFMA kernel runs (csrc/gpt.hip attention_prefill_mfma_k), the per-row kernel below that */
int ctts_k_attention_prefill(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, float* out, int32_t q_per_b,
                             int32_t slot0, const int32_t* kv_start, int32_t M, void* stream);
/* the same with the output type and the slot-pool map of the prompt pass: out_bf16 0 = f32 [M,768], 1 = bf16 [M,768] row-major (what the
 * perf mode's o_proj reads); row_map [M / q_per_b] or NULL: row group -> utterance slot of the cache, kv_start indexed by that slot.
 * Refuses null pointers, out_bf16 outside {0, 1}, q_per_b < 2 (q_per_b == 1 is a decode launch) and a chunk beyond the cmax cache rows. */
int ctts_k_attention_prefill_ex(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, void* out, int32_t out_bf16,
                                int32_t q_per_b, int32_t slot0, const int32_t* kv_start, const int32_t* row_map, int32_t M, void* stream);
/* decode attention of the perf mode: one query row per utterance, bf16 KV cache [slots,12,cmax,64], output bf16 in the fragment-packed
 * order of csrc/decode.hip; desc [M][4] int32 = {utterance slot (-1: skip), KV slot of the query, RoPE position (unused here), first
 * visible key}; n_active: device scalar or NULL (M).  n_cu > 0 with part ([n_cu][8][66] f32) and cnt ([n_cu] int32, zeroed) turns on
 * remainder splitting of the (utterance, head) units over workgroups (csrc/gpt.hip attention_k); n_cu = 0: one workgroup per unit. */
int ctts_k_attention_dec(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, uint16_t* out_packed,
                         const int32_t* desc, const int32_t* n_active, int32_t M, float* part, int32_t* cnt, int32_t n_cu, void* stream);
/* Decode attention of EITHER mode the way the decode step launches it (round 5): kv_dtype CTTS_BF16 = bf16 cache, bf16 output in the
 * fragment-packed order of csrc/decode.hip; CTTS_F32 = f32 cache, f32 output in the packed order of csrc/decode32.hip; 2 = f32 cache, output as
 * hi | lo bf16 planes in decode.hip's order, the lo plane ceil16(M) * 768 elements behind (the split-bf16 parity mode, csrc/decode32x.hip).  covers_all != 0:
 * desc is valid for all M rows (absent rows carry slot -1) and n_active is not read.  Runs the persistent grid (csrc/gpt.hip
 * attention_persist_k: <= one workgroup per CU walking the live (utterance, head) units) unless ctts_k_attention_cfg / CTTS_ATT_PERSIST=0
 * selected one workgroup per unit (attention_k); both give the same bits.  Reference op: examples/onnx/modeling_llama.py:455-475. */
int ctts_k_attention_dec2(const float* qkv, const void* kcache, const void* vcache, int32_t kv_dtype, int32_t cmax, void* out_packed,
                          const int32_t* desc, const int32_t* n_active, int32_t covers_all, int32_t M, void* stream);
/* tests / probes: decode attention launch shape of this process -- persist 0 | 1 (< 0: keep), workgroups of the persistent grid (<= 0:
 * keep; default = the device's CU count), KV blocks per wave ring 2 | 3 | 4 (<= 0: keep; default 4).  Never changes a result bit. */
int ctts_k_attention_cfg(int32_t persist, int32_t workgroups, int32_t ring);
/* round 5 A/B: `hpw` consecutive heads of one utterance per decode-attention workgroup (1 = the shipped grid of one workgroup per (utterance,
 * head); 2 | 3 | 4: the same 4-wave units, 12 / hpw workgroups of 4 hpw waves per utterance -- bit-identical output; env CTTS_ATT_HPW). */
int ctts_k_attention_heads_per_wg(int32_t hpw);
/* The same attention with o_proj + residual folded in (ctts_gpt_weights.wo_hd): wo_hd [12][8][768][8] bf16; part [ceil16(M)][12][768]
 * f32 scratch; cnt [M] int32, zero (left zero); x32 [M][768] f32 residual, updated in place; xp its bf16 copy in the fragment-packed
 * order; ssq [M][48] partial sums of squares of the new residual. */
int ctts_k_attention_oproj(const float* qkv, const uint16_t* kcache, const uint16_t* vcache, int32_t cmax, const uint16_t* wo_hd,
                           const int32_t* desc, const int32_t* n_active, int32_t M, float* part, int32_t* cnt, float* x32, uint16_t* xp,
                           float* ssq, void* stream);
/* what the library's per-call device guard does for `stream`: the device current before the call, the one that owns the stream, the one
 * current inside the guard, whether it switched; fails if the previous device is not restored */
int ctts_k_device_guard_probe(void* stream, int32_t* before, int32_t* stream_dev, int32_t* inside, int32_t* switched);
int ctts_k_embed_codes(const float* emb_code, const int64_t* ids_buf, int32_t tcap, const int32_t* len, float* x, int32_t B, void* stream);
/* The first kernel of a decode step with everything it can produce (csrc/gpt.hip embed_codes_k; n_text > 0: embed_text_k over emb [n_text, 768]):
 * the residual rows x [B, 768], their 16-bit copy xb (row-major bf16; xb_packed: the fragment-packed order of csrc/decode.hip; with
 * xb_lo_plane > 0: hi | lo' fp16 planes of the split-fp16 format, the lo plane xb_lo_plane elements behind), ssq [B, 48] partial sums of
 * squares, xp32 (packed f32 order of csrc/decode32.hip), and per compact row m: desc [B][4] int32 = {utterance (-1: finished), KV slot, RoPE
 * position, first visible key}, rope_cs [B][64] = cos[32] | sin[32] of the row's position out of the [max_pos][32] tables.  Rows: row_map_out
 * != NULL: device-side compaction -- row m is the m-th utterance (in `order`, or ascending) whose finish byte is 0, written to row_map_out[m],
 * the live count to *n_active_out; else the host's row_map (NULL: identity) and *n_active (NULL: B).  zero_p: zero_n words, zero_stride ints
 * apart, set to 0.  Every output pointer may be NULL except x. */
int ctts_k_step_prep(const float* emb, int32_t n_text, const int64_t* ids_buf, int32_t tcap, const int32_t* len, float* x, uint16_t* xb, float* ssq,
                     int32_t B, const int32_t* row_map, const int32_t* n_active, int32_t* desc, const int32_t* kv_start, const uint8_t* finish,
                     int32_t xb_packed, float* xp32, int64_t xb_lo_plane, int32_t* row_map_out, int32_t* n_active_out, const int32_t* order,
                     float* rope_cs, const float* cos_tab, const float* sin_tab, int32_t* zero_p, int32_t zero_n, int32_t zero_stride,
                     void* stream);
/* parity-mode prompt pass: x [M, 768] -> xp32 (packed f32 order) and desc [M][4] of prompt row m: utterance row_map ? row_map[m / q_per_b]
 * : m / q_per_b, KV slot slot0 + m % q_per_b (csrc/gpt.hip prefill_prep32_k) */
int ctts_k_prefill_prep32(const float* x, float* xp32, int32_t* desc, int32_t q_per_b, int32_t slot0, const int32_t* kv_start,
                          const int32_t* row_map, int32_t M, void* stream);
/* prompt pass over the valid tokens only: emb [B, T, 768] -> consecutive rows of x (utterance b's slots kv_start[b] .. T-1), their desc, and
 * last_row [B] (csrc/gpt.hip prefill_compact_k).  Every utterance needs at least one valid token: kv_start[b] < T. */
int ctts_k_prefill_compact(const float* emb, float* x, int32_t* desc, int32_t* last_row, int32_t B, int32_t T, const int32_t* kv_start,
                           void* stream);
/* prompt-pass projection of the f32 parity mode (csrc/prefill32.hip), operands as ctts_k_gemm_dec32: epi 1 = C = res + acc and Cp, 2 =
 * SiLU(gate)*up -> Cp, 100 = RoPE + KV append from desc [M][4] into float32 caches [slots, 12, cmax, 64] (N = 2304, K = 768, q/k weight rows
 * in engine.py `rope_row_perm` order; q -> C).  norm_w != NULL (K = 768): RMSNorm prologue, 1 / rms of the rows of X goes through rstd [M]. */
int ctts_k_gemm_pre32(const float* Ap, const float* Wp, int32_t M, int32_t N, int32_t K, const float* X, int32_t ldx, const float* norm_w,
                      float eps, float* rstd, int32_t epi, float* C, int32_t ldc, const float* res, int32_t ldr, float* Cp, int32_t kch_out,
                      const int32_t* desc, const float* cos_tab, const float* sin_tab, float* kcache, float* vcache, int32_t cmax, void* stream);
/* the fused RMSNorm + QKV + RoPE + KV append launch of the parity decode step, given descriptors: x3 = 0: csrc/decode32.hip (Ap / Wp packed
 * f32, X + norm_w the RMSNorm prologue; bit-identical to ctts_k_gemm + ctts_k_rope_append); x3 = 1: csrc/decode32x.hip (Ap / Wp hi planes, the
 * lo planes a_plane / w_plane elements behind, gain folded into W, 1 / rms from ssq_in or else from X; rope_cs [M][64] replaces the tables) */
int ctts_k_qkv_rope32(int32_t x3, const void* Ap, int64_t a_plane, const void* Wp, int64_t w_plane, int32_t M, const int32_t* n_active,
                      const float* X, int32_t ldx, const float* norm_w, const float* ssq_in, float eps, float* qkv, const int32_t* desc,
                      const float* rope_cs, const float* cos_tab, const float* sin_tab, float* kcache, float* vcache, int32_t cmax,
                      int32_t force_mb, void* stream);
int ctts_k_final_norm(const float* x, int32_t q_per_b, const float* w, float eps, float* hfin, float* hiddens, int32_t max_new,
                      const int32_t* len, int32_t T, int32_t B, void* stream);
int ctts_k_sample(const ctts_gen_state* s, const float* logits, void* stream);
/* the refine-text sampler alone (sample_text_k, gpt.py:439-440,477-525): logits [B, n_text], q [nq, B, n_text], temperature[0], ONE
 * sampling row per utterance, the token replicated over the 4 slots; no repetition penalty */
int ctts_k_sample_text(const ctts_gen_state* s, const float* logits, int32_t n_text, void* stream);
/* The readers of the row descriptors at the end of a decode step, kernel by kernel (tests/test_gpu_step_back.py).
 * ctts_k_final_norm_rows: ctts_k_final_norm with the rest of final_norm_k's arguments -- row_map (compact row -> utterance, NULL: identity),
 * n_active (device scalar, q_per_b = 1 only; NULL: B rows), prompt_len [slots] (NULL: T for all), hfin_packed (the same rows in the packed
 * f32 order of csrc/decode32.hip, or NULL), last_row [B] (row of utterance m's last prompt token after ctts_k_prefill_compact, or NULL). */
int ctts_k_final_norm_rows(const float* x, int32_t q_per_b, const float* w, float eps, float* hfin, float* hiddens, int32_t max_new,
                           const int32_t* len, int32_t T, int32_t B, const int32_t* row_map, const int32_t* n_active, const int32_t* prompt_len,
                           float* hfin_packed, const int32_t* last_row, void* stream);
/* final RMSNorm + hidden capture + heads as the decode step launches them (csrc/decode32.hip gemm_dec32_fnorm16_k, K = 768): Ap = the
 * UN-normalised rows, Wp = the heads, both in the packed f32 order (N padded to a multiple of 16, n_cols columns exist); C [M, ldc] row-major;
 * hid [slots, hid_cap, 768] != NULL: row m's normalised row also goes to hid[desc[m].b][desc[m].slot + 1 - (prompt_len ? prompt_len[b] : T)]
 * when desc[m].b >= 0 and that index is in [0, hid_cap).  ctts_k_dec32_last_variant() says "fnorm16" afterwards. */
int ctts_k_fnorm_heads(const float* Ap, const float* Wp, int32_t M, int32_t N, int32_t n_cols, const int32_t* n_active, const float* norm_w,
                       float eps, float* C, int32_t ldc, const int32_t* desc, float* hid, int32_t hid_cap, int32_t T, const int32_t* prompt_len,
                       void* stream);
/* ctts_k_sample (n_text > 0: ctts_k_sample_text) on COMPACT rows: a grid of `rows` <= s->B logits rows; row m samples utterance desc[m].b at
 * length desc[m].slot + 1 (b = -1: the row does not exist), or without desc utterance row_map[m] (NULL: m) while m < *n_active (NULL: rows).
 * x != NULL (codes only, needs desc, desc_out and kv_start): the next step's first kernel folded into the launch (csrc/kernels.hpp
 * EmbedNext) -- emb_code [4, 626, 768] and the outputs x, xb, ssq, desc_out, xb_packed, xp32, xb_lo_plane, rope_cs as ctts_k_step_prep. */
int ctts_k_sample_rows(const ctts_gen_state* s, const float* logits, int32_t n_text, int32_t rows, const int32_t* row_map, const int32_t* n_active,
                       const int32_t* desc, const float* emb_code, float* x, uint16_t* xb, float* ssq, int32_t* desc_out, const int32_t* kv_start,
                       int32_t xb_packed, float* xp32, int64_t xb_lo_plane, float* rope_cs, const float* cos_tab, const float* sin_tab,
                       void* stream);
/* the device generator's Exp(1) draws (ctts_gen_state.rng_device) of sampling rows row0 .. row0+rows-1 at generation step `step`
 * as a [rows, V] float32 tensor -- distribution tests */
int ctts_k_exp_draws(uint64_t seed, int32_t step, int32_t row0, int32_t rows, int32_t V, float* out, void* stream);
int ctts_k_dwconv_ln(const float* x, const float* w, const float* b, const float* ln_w, const float* ln_b, float eps, int32_t dil,
                     float* y, int32_t B, int32_t F, void* stream);
/* the whole depthwise conv + LayerNorm launcher (kernel tests): C = 512 | 256; yp != NULL: the normalised rows go out as planes in the
 * codec GEMMs' fragment order instead of to y (C = 512 only) -- hi | lo bf16 planes [rows/32][C/16][2][64][8], or with plane_f16 ONE
 * fp16 plane [rows/32][C/16][64][8]; seg != NULL: B = 1 and the F frames are packed segments, seg = device int32 [F][2], frame f's
 * segment [lo, hi) (C = 512 only).  Returns -1 with a message when the launcher refuses the combination; nothing is launched then. */
int ctts_k_dwconv_ln_ex(const float* x, const float* w, const float* b, const float* ln_w, const float* ln_b, float eps, int32_t dil,
                        float* y, int32_t B, int32_t F, int32_t C, uint16_t* yp, int32_t plane_f16, const int32_t* seg, void* stream);
int ctts_k_layernorm(const float* x, const float* w, const float* b, float eps, float* y, int32_t rows, void* stream);
int ctts_k_istft(const float* head, const float* window, const float* twiddle, float* frames, float* wav, int32_t B, int32_t F, void* stream);
/* The Vocos tail's launchers alone (csrc/kernels.hpp: launch_istft_ragged, launch_gather_windows, launch_crop_pcm16_windows,
 * launch_chunks_pcm16), with their arguments in their order and NO checks beyond null pointers: every bound is the caller's.
 * istft_ragged: head [F_total][1026] of packed segments, tok_off [n_seg + 1] device token offsets (2 frames per token), segment i's
 * waveform at wav + 256 (2 tok_off[i] - i), frames [F_total][1024] scratch.  gather_windows: the rows of `win` (device) out of the store
 * into packed [total_rows][768], tok_off [n_win + 1].  crop_pcm16_windows / chunks_pcm16: the last launch of ctts_codec_decode_windows /
 * ctts_codec_decode_windows_rate over a given waveform -- `out` int16 or (out_f32) float32, sum ceil8(n_i) elements; `keep` may be NULL. */
int ctts_k_istft_ragged(const float* head, const float* window, const float* twiddle, float* frames, float* wav, const int32_t* tok_off,
                        int32_t n_seg, int32_t F_total, int32_t F_max, void* stream);
int ctts_k_gather_windows(const float* hid, int64_t slot_stride, int64_t row_stride, const ctts_window* win, int32_t n_win, int32_t total_rows,
                          float* packed, int32_t* tok_off, void* stream);
int ctts_k_crop_pcm16_windows(const float* wav, const ctts_window* win, int32_t n_win, int32_t out_f32, int32_t product, float keep_thr,
                              void* out, uint8_t* keep, void* stream);
int ctts_k_chunks_pcm16(const float* wav, const float* chunks, const ctts_window* win, const ctts_rs_window* rs, int32_t n_win, int32_t out_f32,
                        int32_t product, float keep_thr, void* out, uint8_t* keep, void* stream);
/* The full DVAE's own kernels alone (csrc/dvae.hip).  stft_mag: wav [n] -> mag [F][516] (513 bins of |stft(center, reflect, hann)|, then
 * 3 zero columns), window [1024], twiddle [512][2] as ctts_dvae_weights; refused, with nothing launched, unless n > 512 and
 * F == 1 + n / 256.  gfsq_encode: feat [rows][1024] -> codes [rows][4] int32; gfsq_embed: codes [rows][4] int64 -> feat [rows][1024];
 * both read the quantiser's weights and levels as ctts_dvae_create marshalled them into the engine `c`. */
int ctts_k_stft_mag(const float* wav, int32_t n, const float* window, const float* twiddle, float* mag, int32_t F, void* stream);
int ctts_k_gfsq_encode(ctts_dvae* c, const float* feat, int32_t* codes, int32_t rows, void* stream);
int ctts_k_gfsq_embed(ctts_dvae* c, const int64_t* codes, float* feat, int32_t rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
