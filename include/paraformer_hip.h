/*
 * paraformer_hip.h — C ABI of libparaformer_hip.so
 *
 * MI355X (gfx950) native replacement for the two native engines behind the
 * reference's offline path (manyeyes/AliParaformerAsr; citations are relative
 * to that repository's root):
 *
 *   - Microsoft.ML.OnnxRuntime  InferenceSession.Run  (encoder + CIF + decoder)
 *       call sites AliParaformerAsr/OfflineProjOfParaformer.cs:68,
 *                  AliParaformerAsr/OfflineProjOfSenseVoiceSmall.cs:156,
 *                  AliParaformerAsr/OfflineProjOfSeacoParaformer.cs:116
 *   - ManySpeech.SpeechFeatures OnlineFbank.GetFbank  (kaldi fbank)
 *       call site  AliParaformerAsr/WavFrontend.cs:21-27,35
 *
 * plus the managed hot loops around them (LFR/CMVN WavFrontend.cs:53-111,
 * PadSequence Utils/PadHelper.cs:23-65, arg-max OfflineRecognizer.cs:139-152,
 * CIF-peak timestamps OfflineRecognizer.cs:200-302).
 *
 * Conventions
 *   - plain C types only; the caller allocates and pins every in/out buffer;
 *     the library never retains a caller pointer past return;
 *   - every function returns PF_OK (0) or a negative pf_status; the message is
 *     available from pf_last_error() (thread-local);
 *   - calls on one handle are serialised internally (one HIP stream per
 *     handle); different handles may be used from different threads;
 *   - there is no CPU fallback: without a usable gfx950 device pf_create
 *     fails with PF_ERR_DEVICE.
 *
 * The reference-side binding for each entry point (C# P/Invoke) is shown in
 * INTEGRATION.md.
 */
#ifndef PARAFORMER_HIP_H_
#define PARAFORMER_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 6

typedef enum pf_status {
  PF_OK = 0,
  PF_ERR_INVALID_ARG = -1,   /* null pointer, bad size; C# maps to ArgumentException          */
  PF_ERR_DEVICE = -2,        /* no gfx950 device / HIP runtime error                          */
  PF_ERR_IO = -3,            /* file missing or unreadable                                    */
  PF_ERR_FORMAT = -4,        /* malformed .pfw / am.mvn / yaml / tokens                       */
  PF_ERR_CAPACITY = -5,      /* caller buffer too small (required size is reported)           */
  PF_ERR_UNSUPPORTED = -6,   /* model kind / option not built                                 */
  PF_ERR_DISPOSED = -7,      /* handle used after dispose (ObjectDisposedException)           */
  PF_ERR_TOKENS = -8,        /* "tokens invalid" (OfflineRecognizer.cs:30-33)                 */
  PF_ERR_NULL_SAMPLES = -9,  /* ArgumentNullException("source") (WavFrontend.cs:34)           */
  PF_ERR_RECOGNITION = -10   /* "Offline recognition failed" (OfflineRecognizer.cs:194-197)   */
} pf_status;

int pf_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* pf_last_error(void);

/* ------------------------------------------------------------------------ */
/* 1. Engine handle: replaces OfflineModel (ORT session, OfflineModel.cs:35-70)
 *    + the per-stream WavFrontend state (WavFrontend.cs:18-29).              */
/* ------------------------------------------------------------------------ */
typedef struct pf_engine pf_engine;

typedef struct pf_engine_config {
  int32_t struct_size;        /* = sizeof(pf_engine_config)                                   */
  int32_t device;             /* HIP device ordinal                                           */
  /* weights: exactly one of the three sources (PFW1 container, see weights.py) */
  const char* weights_path;   /* file                                                          */
  const void* weights_host;   /* host image                                                    */
  const void* weights_device; /* device image (e.g. landed by an RCCL broadcast); not copied,
                                 must outlive the engine                                       */
  int64_t weights_bytes;      /* size of the host/device image                                 */
  /* CMVN: am.mvn path (WavFrontend.cs:112-153) or explicit vectors            */
  const char* mvn_path;
  const float* cmvn_shift;    /* <AddShift> vector                                             */
  const float* cmvn_scale;    /* <Rescale> vector                                              */
  int32_t cmvn_dim;           /* 560                                                           */
  /* FrontendConfEntity (Model/FrontendConfEntity.cs:7-15); 0 / NULL = reference default,
     except dither whose default is carried explicitly                         */
  int32_t fs;                 /* 16000                                                         */
  int32_t n_mels;             /* 80                                                            */
  int32_t lfr_m;              /* 7                                                             */
  int32_t lfr_n;              /* 6                                                             */
  int32_t snip_edges;         /* 0 (false)                                                     */
  float dither;               /* kaldi dither: N(0,1) * dither added to every sample of every frame
                                 (reference default 1.0, Model/FrontendConfEntity.cs:12); drawn on the
                                 device from a counter-based generator seeded by dither_seed          */
  const char* window;         /* "hamming"                                                     */
  int32_t use_itn;            /* SenseVoice: conf.use_itn (OfflineRecognizer.cs:27)            */
  int32_t frame_length_ms;    /* 0 = 25; anything but 25 -> PF_ERR_UNSUPPORTED                 */
  int32_t frame_shift_ms;     /* 0 = 10; anything but 10 -> PF_ERR_UNSUPPORTED                 */
  int32_t dither_seed;        /* seed of the dither stream (same seed + same audio = same features) */
  int32_t math_mode;          /* 0 = f16 operands on the MFMA (default); 1 = fp32 MFMA parity mode
                                 (v_mfma_f32_32x32x2_f32: exact fp32 products, ~1/16 of the speed); 2 = the arithmetic
                                 of the reference's default model.int8.onnx (Examples/Program.cs:98-101): every
                                 Linear as DynamicQuantizeLinear + MatMulInteger on v_mfma_i32_32x32x32_i8, weights
                                 quantised per output channel as onnxruntime's quantize_dynamic does; 3 = "exact" at
                                 matrix-core speed (ABI 5): the fp32 graph of mode 1 with every large Linear as three
                                 f16 MFMA products of (hi, 2^11 lo) operand pairs — 22 mantissa bits per operand, fp32
                                 accumulation — and fp32-MFMA flash attention */
  int32_t reserved[3];
} pf_engine_config;

int pf_engine_create(const pf_engine_config* cfg, pf_engine** out);
/* Idempotent teardown (Dispose(bool) pattern, OfflineRecognizer.cs:448-476: Dispose() and a later finaliser
   may both call it); waits for a call in flight on another thread.  Later calls on the handle -> PF_ERR_DISPOSED. */
void pf_engine_destroy(pf_engine* e);

/* Model facts the managed side needs. */
int pf_engine_info(pf_engine* e, int32_t* kind /*0 paraformer,1 sensevoice,2 seaco*/,
                   int32_t* vocab, int32_t* feat_dim, int32_t* has_timestamp_head);

/* ------------------------------------------------------------------------ */
/* 2. Seam "WavFrontend": GetFbank + LfrCmvn (WavFrontend.cs:31-51), called
 *    from OfflineStream.AddSamples (OfflineStream.cs:40-41).                 */
/* ------------------------------------------------------------------------ */
/* Number of LFR frames the front-end yields for n samples (floor(T80/lfr_n), quirk Q1). */
int pf_frontend_num_frames(pf_engine* e, int64_t n_samples, int32_t* t_lfr_out);
/* samples in [-1,1] -> feats [T, lfr_m*n_mels] (row-major, float32).
   feats_cap = capacity of feats_out in floats. samples == NULL -> PF_ERR_NULL_SAMPLES. */
int pf_frontend(pf_engine* e, const float* samples, int64_t n_samples,
                float* feats_out, int64_t feats_cap, int32_t* t_lfr_out);
/* kaldi fbank only: [T80, n_mels] (OnlineFbank.GetFbank, WavFrontend.cs:35). */
int pf_fbank(pf_engine* e, const float* samples, int64_t n_samples,
             float* fbank_out, int64_t fbank_cap, int32_t* t80_out);

/* ------------------------------------------------------------------------ */
/* 3. Seam "IOfflineProj.ModelProj" (+ arg-max): IOfflineProj.cs:38,
 *    OfflineProjOfParaformer.cs:39-87, OfflineRecognizer.cs:139-152.         */
/* ------------------------------------------------------------------------ */
typedef struct pf_batch_out {
  int32_t struct_size;
  /* capacities (in) */
  int32_t l_cap;              /* token slots per utterance in token_ids                        */
  int64_t logits_cap;         /* floats available in logits (0 = do not return logits)         */
  int64_t cif_peak_cap;       /* floats available in cif_peak (0 = skip)                       */
  /* outputs */
  int64_t* token_ids;         /* [B, l_cap] arg-max ids, first L valid per row; ties -> larger
                                 index (quirk Q4); all L positions kept (quirk Q5)             */
  int32_t* token_num;         /* [B] model_out_lens (floor(sum alpha)); unused by reference    */
  float* logits;              /* [B, L, V] log-probs (model_out), optional                     */
  float* cif_peak;            /* [B, 3*Tmax] us_cif_peak, optional (timestamp models)          */
  int32_t L;                  /* out: decoder positions per utterance (logits dim 1)           */
  int32_t V;                  /* out: vocabulary (logits dim 2)                                */
  int32_t cif_peak_len;       /* out: 3*Tmax or 0                                              */
  int32_t reserved;
} pf_batch_out;

/* `speech` is the tensor the reference hands to ORT: [B, Tmax, feat_dim] float32,
   already padded and sentinel-substituted (PadHelper.cs:63); speech_lengths is
   Tmax for every row (quirk Q2) and therefore not a parameter.
   hotwords: SeACo only, int32 [n_hotwords, 10] (EmbedSeacoModel.cs:70-123), may be NULL. */
int pf_forward_feats(pf_engine* e, const float* speech, int32_t B, int32_t Tmax,
                     const int32_t* hotwords, int32_t n_hotwords, pf_batch_out* out);

/* ModelProj including PadSequence: B ragged feature buffers (OfflineInputEntity.Speech,
   SpeechLength = float count each) -> padded on device, sentinel applied, forward. */
int pf_model_proj(pf_engine* e, const float* const* speech, const int32_t* speech_len_floats,
                  int32_t B, const int32_t* hotwords, int32_t n_hotwords, pf_batch_out* out);

/* ------------------------------------------------------------------------ */
/* 4. Fused fast path: raw audio in, ids out (AddSamples + GetResults numeric
 *    part in one device pipeline).                                           */
/* ------------------------------------------------------------------------ */
int pf_recognize(pf_engine* e, const float* const* samples, const int64_t* n_samples,
                 int32_t B, const int32_t* hotwords, int32_t n_hotwords, pf_batch_out* out);

/* Split form used by the benchmark so that the timed region starts with the audio
   resident in HBM: stage (H2D) -> run (device only, async on the engine stream) ->
   fetch (D2H of ids). */
int pf_stage_audio(pf_engine* e, const float* const* samples, const int64_t* n_samples, int32_t B);
/* SeACo: hotword ids [n_hotwords, 10] (PadList output, EmbedSeacoModel.cs:70-123) used by the following
   pf_run_staged calls (the other forward entry points take them per call); ignored by other model kinds. */
int pf_engine_set_hotwords(pf_engine* e, const int32_t* hotwords, int32_t n_hotwords);
int pf_run_staged(pf_engine* e);      /* enqueues the whole pipeline, returns after the CIF
                                         length read-back (the path's only host sync)          */
int pf_sync(pf_engine* e);            /* waits for the engine stream                           */
/* Copies the results of the calling THREAD's last pf_forward_feats / pf_model_proj / pf_recognize (kept per
   thread, so the two-call protocol — first call learns L and V, pf_fetch fills right-sized buffers — is safe
   with concurrent callers on one engine; calls themselves are serialised by an internal mutex, like the
   reference's static lock, OfflineStream.cs:19).  After pf_run_staged it returns the staged result (the
   staged API is engine state: one caller at a time). */
int pf_fetch(pf_engine* e, pf_batch_out* out);
/* The hypotheses of the staged result WITHOUT leaving the device (ABI 4): writes ids [B, l_cap] int64 (columns >= L
   filled with -1) into `ids_dev` (device memory of the engine's GPU) on the engine stream and waits for it, so a caller
   that gathers hypotheses across GPUs (RCCL all-gather over xGMI) hands the buffer straight to the
   collective.  *L_out (optional) receives the decoder length.  PF_ERR_CAPACITY when l_cap < L.  Replaces, for that
   caller, the host copy the reference makes of the logits tensor (OfflineProjOfParaformer.cs:73-79). */
int pf_fetch_ids_device(pf_engine* e, int64_t* ids_dev, int32_t l_cap, int32_t* L_out);

/* ---- Decoding extras (additions to ABI 6; default 0 = the reference behaviour, bit for bit) ------------------------
   pf_engine_set_decode sets flags for the forwards that FOLLOW on this engine (like pf_engine_set_hotwords):
     PF_DECODE_SCORES  keep s[b, l], the log-prob of the arg-max id at every position [B, L] — the value the arg-max
                       compared, (x - max) - log(sum exp(x - max)).  paraformer and SenseVoice, every math_mode.
     PF_DECODE_CTC     implies SCORES.  SenseVoice only.  The CTC collapse the reference leaves commented out
                       (OfflineRecognizer.cs:153-168) runs on the device right behind the arg-max: over the first n_b frames
                       of utterance b a token starts at frame t when y[t] != 0 (blank) and (t == 0 or y[t] != y[t-1]) and
                       extends while y stays equal ("a a _ a b b" -> a, a, b).  Per token: id, first / last frame (indices in
                       the row, prompt rows included) and score = the largest s[t] of its run.
   n_b = 4 + pf_frontend_num_frames(n_samples[b]) for pf_recognize / pf_stage_audio + pf_run_staged,
         speech_len_floats[b] / feat_dim for pf_model_proj, Tmax for pf_forward_feats (no lengths exist there).
   The encoder still runs every row at the batch length (quirk Q2): frame ids of a short utterance depend on its batch
   mates; the collapse only stops reading at n_b.
   PF_ERR_UNSUPPORTED: PF_DECODE_CTC on a paraformer / SeACo model, any flag on a SeACo model.
   The fetch calls read the calling thread's last forward, like pf_fetch — call them BEFORE the pf_fetch that receives
   token_ids (it releases the thread's slot).  PF_ERR_INVALID_ARG when that forward ran without the flag. */
#define PF_DECODE_SCORES 1
#define PF_DECODE_CTC 2
int pf_engine_set_decode(pf_engine* e, int32_t flags);
/* scores [B, L] (NULL: only learn L); PF_ERR_CAPACITY when cap < B * L */
int pf_fetch_scores(pf_engine* e, float* scores, int64_t cap, int32_t* L_out);
/* n [B] token counts and *n_max their maximum (both optional); ids / first / last / score: arrays [B, cap], each
   optional, slots >= n[b] hold -1 / -1 / -1 / 0.  All four NULL: only learn n and n_max.  PF_ERR_CAPACITY when
   cap < n_max (n and n_max are filled in first). */
int pf_fetch_ctc(pf_engine* e, int64_t* ids, int32_t* first, int32_t* last, float* score, int32_t cap, int32_t* n,
                 int32_t* n_max);

/* ---- Top-k and n-best (additions to ABI 6; nothing is launched or allocated without the flag) --------------------------
   PF_DECODE_TOPK (pf_engine_set_decode; implies SCORES; paraformer and SenseVoice, every math_mode; PF_ERR_UNSUPPORTED for
   a SeACo model and for a pf_group forward): behind the arg-max one kernel (csrc/k_topk.hip) selects at every position
   [B, L] the K best entries of the log-prob row y the arg-max scanned — bit for bit the row a logits request returns.
   ORDER: entry a ranks before entry b when y[a] > y[b], or y[a] == y[b] and a > b (of equal values the LARGER index first,
   the reference loop's tie rule; -0.0 == +0.0).  NaN entries are never ranked.  n = min(K, non-NaN entries of the row);
   slots r >= n hold id -1 and value -inf.  For a row without NaN rank 0 is the arg-max id and its value is the
   pf_fetch_scores value of that position (a row with a NaN is all NaN in log-softmax form: n = 0).
   K: pf_engine_set_topk, 1 .. PF_TOPK_MAX, default 4, for the forwards that follow.
   The flag is bit 8: pf_engine_set_decode(e, 4) has been answered with PF_ERR_INVALID_ARG since the decoding extras exist
   and callers (and the decode tests) rely on that answer for an unknown bit, so bit 4 stays unassigned. */
#define PF_DECODE_TOPK 8
#define PF_TOPK_MAX 8
#define PF_NBEST_MAX 64
int pf_engine_set_topk(pf_engine* e, int32_t k);
/* ids [B * L, K] int64, val [B * L, K] fp32, n [B * L] int32 of the calling thread's last forward, each optional; all three
   NULL: only learn *L_out and *K_out.  PF_ERR_CAPACITY when cap_rows < B * L; PF_ERR_INVALID_ARG when that forward ran
   without the flag.  Call it BEFORE the pf_fetch that receives token_ids (it releases the thread's slot). */
int pf_fetch_topk(pf_engine* e, int64_t* ids, float* val, int32_t* n, int64_t cap_rows, int32_t* L_out, int32_t* K_out);
/* The exact n-best list of ONE utterance from its top-k lists (pure host code).  Paraformer positions are independent given
   the audio, so a hypothesis is a rank vector r[0..L) with r[l] < n[l], and r[l] == 0 for l >= n_free =
   min(L, token_num[b]) (positions past the utterance's own token count keep the 1-best id, as the reference does there:
   hypothesis 0 is the existing result id for id).  Its score is the float64 sum of the fp32 values val[l, r[l]] added from
   l = 0 up.  Listed by descending score, ties to the lexicographically smaller rank vector; hypotheses are not
   de-duplicated by text.  ids (optional, unused by the enumeration), val [L, K], n [L]; N: 1 .. PF_NBEST_MAX.
   out_ranks [N, L], out_scores [N], *n_out = how many exist (<= N; 0 when some n[l] == 0).
   PF_ERR_INVALID_ARG for a ranked value that is NaN or +inf. */
int pf_host_nbest(const int64_t* ids, const float* val, const int32_t* n, int32_t L, int32_t K, int32_t n_free, int32_t N,
                  int32_t* out_ranks, double* out_scores, int32_t* n_out);

/* ---- CTC beam search (additions to ABI 6; nothing is launched or allocated without the flag) ---------------------------
   PF_DECODE_CTC_BEAM (pf_engine_set_decode; SenseVoice only, every math_mode; implies TOPK and SCORES; independent of
   PF_DECODE_CTC; PF_ERR_UNSUPPORTED for a paraformer or SeACo model and for a pf_group forward): behind the top-k launch one
   kernel (csrc/k_ctcbeam.hip) runs a CTC prefix beam search per utterance and keeps its N best LABELINGS.  Under CTC the
   probability of a labeling is the sum over all of its alignments; the search sums the alignments it keeps.
   INPUTS per utterance b: the frames t < n_b (the count PF_DECODE_CTC uses, prompt rows included), the blank (id 0) log-prob
   of each frame and the frame's top-k list (K of pf_engine_set_topk) exactly as pf_fetch_topk returns it.  fp32 inputs are
   widened to float64; all scores are float64.  lse(a, b) = max + log1p(exp(-|a - b|)); an argument of -inf gives the other.
   The beam is an ordered list of at most W entries (prefix, pb, pnb), at first [((), 0, -inf)].  At frame t the candidates C_t
   are the listed entries r < n[t] whose id is not blank.  For beam entry i in rank order, last token e, tot = lse(pb, pnb):
     stay     (candidate index i*(K+1)):      pb' = tot + lb[t]; pnb' = pnb + lp_t(e) when the prefix is non-empty and e in C_t,
              else -inf
     extend c (candidate index i*(K+1)+1+r):  pnb' = (c == e ? pb : tot) + lp_t(c), pb' = -inf; dropped when the base is -inf
     merge    prefix + c is the prefix of another beam entry q: no candidate of its own, pnb'_q = lse(pnb'_q, value)
     select   candidates whose total lse(pb', pnb') is -inf are discarded; the W best by total stay, ties to the smaller
              candidate index; that order is the new beam's order.
   After the last frame the first N entries are the hypotheses: ids, length, score = total.  n_hyp[b] = 0 when a frame t < n_b
   has n[t] == 0 or a NaN blank log-prob.  Hypothesis 0 is the search's best, NOT necessarily the collapsed arg-max ids;
   token_ids, pf_fetch_scores, pf_fetch_ctc and pf_fetch_topk are what they are without the flag.
   W / N: pf_engine_set_ctc_beam, 1 <= N <= W <= PF_NBEST_MAX, default 16 / 16, for the forwards that follow.
   The flag is bit 16; bits 4 and 64 stay unassigned (PF_ERR_INVALID_ARG). */
#define PF_DECODE_CTC_BEAM 16
int pf_engine_set_ctc_beam(pf_engine* e, int32_t W, int32_t N);
/* ids [B, N, cap] int64 (-1 past a hypothesis' length), len [B, N] (0 past n_hyp), score [B, N] float64 (-inf past n_hyp),
   n_hyp [B], each optional; N is the one in force at the forward.  *len_max = the longest hypothesis of the batch; ids with
   cap < *len_max -> PF_ERR_CAPACITY (len_max, n_hyp, len and score filled in).  PF_ERR_INVALID_ARG when that forward ran
   without the flag.  Call it BEFORE the pf_fetch that receives token_ids (it releases the thread's slot). */
int pf_fetch_ctc_beam(pf_engine* e, int64_t* ids, int32_t* len, double* score, int32_t cap, int32_t* n_hyp, int32_t* len_max);
/* The same search for ONE utterance in plain host code (the twin of the kernel): blank_lp[t * blank_stride], ids / val [T, K],
   n [T]; out_ids [N, cap], out_len [N], out_score [N] filled as above, *n_hyp.  PF_ERR_CAPACITY when a hypothesis is longer
   than cap (cap >= T always suffices). */
int pf_host_ctc_beam(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int32_t T,
                     int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len, double* out_score,
                     int32_t cap, int32_t* n_hyp);

/* ---- CTC hot words (additions to ABI 6; nothing is launched or allocated without an installed set) ----------------------
   Shallow fusion of a hot-word set into the CTC beam search above: a hypothesis earns a bonus per token while it spells a
   hot word, keeps it when the word completes and loses it when the match breaks.  SenseVoice only; SeACo has its bias decoder.
   INPUTS: everything the beam search takes, a set of H hot words (sequences of ids in [1, V); blank is id 0) and a boost s
   (float32, finite, s >= 0, widened to float64).
   MATCHED TOKENS of a label sequence y: walk y left to right keeping the SEGMENT read since the last completion (empty at the
   start, m = 0).  After each token, if one or more hot words are a suffix of the segment, the longest one completes:
   m += its length and the segment is emptied.  At the end d(y) is the length of the longest suffix of the segment that is a
   PROPER prefix of some hot word (the pending partial match; 0 when there is none).  Matches do not overlap: of the hot
   words `ab` and `abc` only `ab` can ever complete, so a hot-word set should be prefix-free (nothing is special-cased).
     bias(y) = double(s) * (m(y) + d(y))       bonus(y) = double(s) * m(y)
   each ONE float64 product of the widened boost by an integer.
   SEARCH: the beam search above with exactly two changes.
     select   a candidate's key is total + bias(its prefix); a candidate whose total is -inf is still discarded; the W best
              by key stay, ties to the smaller candidate index; the stored pb / pnb remain unbiased (equal prefixes have equal
              bias, so folding a merged extension into the stay candidate stays valid).
     finish   after the last frame each entry gets score = lse(pb, pnb) + bonus(prefix) (the pending part is revoked); the
              entries are re-ordered by descending score, ties to the smaller beam rank; the first N are the hypotheses:
              ids, length, score, matched = m(prefix), loglik_sum = lse(pb, pnb) = the unbiased log of the summed alignments.
   s = 0 or an empty set IS the unbiased search, bit for bit.  Only ids in a frame's top-k list can be boosted (the
   candidates are the K <= 8 listed ids).  The definition in Python is tests/ctcbeam_bias_ref.py.
   AUTOMATON (pf_host_hotword_graph): a trie over the set with Aho-Corasick failure links, compiled into a deterministic
   table.  State 0 is the root.  From state u on token c: col = tok_col[c]; col < 0 (not a hot-word token): root, nothing
   completes; else e = table[u * A + col]: next state e & 0xFFFF, completed length (e >> 16) & 0xFF (then the next state is the root), e >> 24 = depth[next state].
   depth[u] = d of a sequence that ends in u.  *n_states = S (trie nodes, root included), *n_cols = A (distinct hot-word
   tokens); tok_col [V], table [S * A] (table_cap entries), depth [S] (depth_cap entries) are optional: call with NULL to size.
   An empty hot word is dropped, a duplicate is harmless.  PF_ERR_INVALID_ARG: an id <= 0 or >= V.  PF_ERR_CAPACITY: more than
   PF_HOTWORD_STATES_MAX states, a hot word longer than PF_HOTWORD_LEN_MAX ids, a table over PF_HOTWORD_TABLE_BYTES_MAX, or
   table_cap / depth_cap too small (sizes filled in). */
#define PF_HOTWORD_STATES_MAX 4096
#define PF_HOTWORD_LEN_MAX 64
#define PF_HOTWORD_TABLE_BYTES_MAX (16 * 1024 * 1024)
int pf_host_hotword_graph(const int32_t* ids, const int32_t* lens, int32_t n_hotwords, int32_t V, int32_t* n_states, int32_t* n_cols,
                          int32_t* tok_col, int32_t* table, int64_t table_cap, int32_t* depth, int32_t depth_cap);
/* The set of the forwards that FOLLOW on this engine: n_hotwords words, word i = lens[i] ids at ids[sum of the lens before].
   SenseVoice only (PF_ERR_UNSUPPORTED otherwise).  n_hotwords == 0 or boost == 0 (or only empty words) clears it.  The table
   is built and uploaded once here.  With a set installed a forward with PF_DECODE_CTC_BEAM runs the biased search (there is no
   decode bit of its own); pf_fetch_ctc_beam then returns the biased order and score, PF_DECODE_ALIGN aligns those hypotheses;
   token_ids, pf_fetch_scores, pf_fetch_ctc and pf_fetch_topk are what they are without the set.  PF_ERR_INVALID_ARG: a
   negative, infinite or NaN boost, an id outside [1, V); PF_ERR_CAPACITY as pf_host_hotword_graph (the installed set stays). */
int pf_engine_set_ctc_hotwords(pf_engine* e, const int32_t* ids, const int32_t* lens, int32_t n_hotwords, float boost);
/* matched [B, N] int32 (0 past n_hyp) and loglik_sum [B, N] float64 (-inf past n_hyp) of the last forward's hypotheses, each
   optional, in pf_fetch_ctc_beam's order: score - boost * matched == loglik_sum bit for bit.  Slot rules as pf_fetch_ctc_beam
   (call it before the pf_fetch that takes the ids).  PF_ERR_INVALID_ARG when that forward ran unbiased. */
int pf_fetch_ctc_beam_hot(pf_engine* e, int32_t* matched, double* loglik_sum);
/* pf_host_ctc_beam with a hot-word set and a boost: the biased search for ONE utterance in plain host code.  out_matched [N],
   out_loglik [N] next to out_score.  Hot-word ids are in [1, 2^24) here (there is no vocabulary to bound them). */
int pf_host_ctc_beam_hot(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int32_t T,
                         int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len, double* out_score,
                         int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords, float boost,
                         int32_t* out_matched, double* out_loglik);

/* ---- CTC language model (additions to ABI 6; nothing is launched, allocated or uploaded without a model) ----------------
   Shallow fusion of a back-off n-gram language model into the CTC beam search above: the weighted LM score of a prefix is one
   more term of the key the search selects by, so the model decides which prefixes survive a frame.  Opt-in, absent from the
   reference.  The definition in Python is tests/ctcbeam_lm_ref.py.
   THE MODEL: a back-off n-gram LM of order O (1 <= O <= PF_LM_ORDER_MAX) over token ids in [1, V).  Each listed n-gram has a
   float32 natural-log probability, each listed n-gram of order < O may have a float32 natural-log back-off weight; the model
   carries optional bos / eos / unk ids (-1: none; an unk must be a listed unigram), a float32 oov log-probability used when
   there is no unk, and a set of TRANSPARENT ids.  All weights are finite.  n-grams whose prefix context is not listed are legal.
   ONE STEP: g and the context h are functions of the label sequence alone.  Start: g = +0.0, h = (bos) with a bos, else ().
   For each token c in order:
     c transparent: nothing changes (no weight, no bonus, same h).
     c no listed unigram: with an unk, c is replaced by unk for scoring and for the context; else g = (g + alpha * oov) + beta
       and h = ().
     otherwise take h' = the last min(|h|, O - 1) tokens of h and repeat: if h' . c is listed, g = g + alpha * logp(h' . c) and
       stop; else, if h' is listed with a back-off, g = g + alpha * bo(h'); drop the first token of h' (the empty context ends
       the walk at the unigram).  Then g = g + beta.  The new h is the longest suffix of h . c that is a listed n-gram of
       order < O.
   alpha >= 0 and beta are finite float32; every operand is widened to float64; alpha * x is the (exact) product of two widened
   floats and every + one rounded float64 addition in exactly this order.  The definition, the host scorer and the kernels
   give bit-equal g.  END OF SENTENCE: with PF_LM_EOS and an eos id one more step for eos, without beta, ends a hypothesis.
   SEARCH: the beam search above (with the hot-word changes when a set is given) and one more term.
     select   key = (total + boost * (m + d)) + g(prefix), the hot-word term only with a set; a candidate whose total is -inf
              is still discarded; the W best by key stay, ties to the smaller candidate index; pb / pnb stay unfused.
     finish   score = (lse(pb, pnb) + boost * m) + g_final; re-ordered by descending score, ties to the smaller beam rank;
              per hypothesis ids, length, score, loglik_sum = lse(pb, pnb), lm_sum = g_final (and matched with hot words):
              score == (loglik_sum + boost * matched) + lm_sum bit for bit.
   alpha = beta = 0 gives the unfused lists and scores bit for bit.  Only ids in a frame's top-k list are candidates.
   THE IMAGE: pf_host_lm_build compiles the model into one flat image of a back-off automaton: state 0 is the empty context
   with a dense [V] lookup, every other state has an arc list sorted by token, a back-off state and weight, and next states
   are precomputed.  Its layout is private (csrc/lm_dev.h).
   OUT OF SCOPE HERE: a paraformer has a position-synchronous search of its own that takes the same model (see "N-best
   search"; pf_engine_set_ctc_lm keeps refusing it); SeACo, pf_group forwards, neural LMs, binary LM formats. */
#define PF_LM_ORDER_MAX 8
#define PF_LM_IMAGE_BYTES_MAX (1024 * 1024 * 1024)
#define PF_LM_EOS 1
typedef struct pf_lm pf_lm;
/* n_ngrams [order]; then per listed n-gram, all 1-grams first, then all 2-grams, ...: its k ids in `ids` (flattened), logp and
   backoff (NaN: listed without a back-off weight; not read at the highest order); transparent: n_transparent ids in [0, V).
   PF_ERR_INVALID_ARG: a duplicate n-gram, an id outside [1, V), a non-finite weight, an unk that is no listed unigram;
   PF_ERR_CAPACITY: an image over PF_LM_IMAGE_BYTES_MAX.  *lm is released with pf_lm_free. */
int pf_host_lm_build(int32_t order, const int64_t* n_ngrams, const int32_t* ids, const float* logp, const float* backoff, int32_t V,
                     int32_t bos, int32_t eos, int32_t unk, float oov, const int32_t* transparent, int32_t n_transparent, pf_lm** lm);
/* ARPA text against a token table (V = n_tokens).  Section counts are checked; each value is float32(strtod(text) * ln 10);
   words map to ids by exact equality with the table (the first spelling wins); <s>, </s> and <unk> are recognised by spelling;
   an n-gram with a word that is not in the table (or is id 0) is dropped and counted in *n_dropped (optional); every token
   spelled <|...|> is transparent.  PF_ERR_INVALID_ARG with path:line for a malformed or truncated file, PF_ERR_IO when it
   cannot be opened. */
int pf_host_lm_from_arpa(const char* path, const char* const* tokens, int32_t n_tokens, float oov, int64_t* n_dropped, pf_lm** lm);
/* each optional */
int pf_host_lm_info(const pf_lm* lm, int32_t* order, int64_t* n_states, int64_t* n_arcs, int64_t* image_bytes);
/* The plain walk: *g and *state after ids[0 .. n) from the start (PF_LM_EOS in flags: and the end-of-sentence step);
   g_pos / state_pos [n]: after every token.  All four optional. */
int pf_host_lm_score(const pf_lm* lm, const int32_t* ids, int32_t n, float alpha, float beta, int32_t flags, double* g, int32_t* state,
                     double* g_pos, int32_t* state_pos);
void pf_lm_free(pf_lm* lm);
/* The model of the forwards that FOLLOW on this engine.  SenseVoice only (PF_ERR_UNSUPPORTED otherwise).  lm = NULL clears.  The
   engine takes a reference of its own (pf_lm_free may follow at once) and uploads the image once, into a buffer of its own; a
   call with the same model only updates alpha / beta / flags.  With a model installed a forward with PF_DECODE_CTC_BEAM runs
   the fused search (there is no decode bit of its own), together with the hot-word set when one is installed;
   pf_fetch_ctc_beam then returns the fused order and score, PF_DECODE_ALIGN aligns those hypotheses; token_ids, pf_fetch_scores,
   pf_fetch_ctc and pf_fetch_topk are what they are without the model.  PF_ERR_INVALID_ARG: alpha negative or not finite, beta
   not finite, an unknown flag (the installed model stays). */
int pf_engine_set_ctc_lm(pf_engine* e, const pf_lm* lm, float alpha, float beta, int32_t flags);
/* lm_sum [B, N] float64 (0 past n_hyp) and loglik_sum [B, N] float64 (-inf past n_hyp) of the last forward's hypotheses, each
   optional, in pf_fetch_ctc_beam's order: score == (loglik_sum + boost * matched) + lm_sum bit for bit (matched: with a
   hot-word set, pf_fetch_ctc_beam_hot).  Slot rules as pf_fetch_ctc_beam (call it before the pf_fetch that takes the ids).
   PF_ERR_INVALID_ARG when that forward ran without a model. */
int pf_fetch_ctc_beam_lm(pf_engine* e, double* lm_sum, double* loglik_sum);
/* pf_host_ctc_beam_hot plus the model, alpha, beta and flags: the fused search for ONE utterance in plain host code.  An empty
   hot-word set (n_hotwords == 0 or boost == 0) is allowed: out_matched is then 0.  out_lm [N] (0 past n_hyp) next to out_loglik. */
int pf_host_ctc_beam_lm(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int32_t T,
                        int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len, double* out_score,
                        int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords, float boost,
                        int32_t* out_matched, double* out_loglik, const pf_lm* lm, float alpha, float beta, int32_t flags, double* out_lm);

/* ---- N-best search (additions to ABI 6; nothing is launched, allocated or uploaded without pf_engine_set_nbest_search) ----
   A position-synchronous beam search over a paraformer's per-position top-k lists, on the device (csrc/k_nbestsearch.hip), one
   launch per batch, with optional hot-word and n-gram LM shallow fusion.  pf_host_nbest above is exact only because positions
   are independent; a language model couples them, so the fused n-best is no re-ranking of the acoustic one: the model decides
   which prefixes survive a position.  Opt-in, absent from the reference.  The definition in Python is tests/nbest_search_ref.py.
   INPUTS per utterance: the top-k block exactly as pf_fetch_topk returns it (ids [L, K], val [L, K] float32, n [L]);
   n_free = min(L, max(token_num, 0)); 1 <= N <= W <= PF_NBEST_MAX, K <= PF_TOPK_MAX; optionally a hot-word set with a boost s
   (automaton, m, d, bias and bonus as in "CTC hot words", read over an id sequence) and a model with alpha, beta and flags (g,
   the context, PF_LM_EOS, transparent ids, unk and oov as in "CTC language model").  fp32 inputs are widened; all scores are
   float64; alpha * x and s * integer are exact products and every + is ONE rounded addition in the order written; nothing
   transcendental is evaluated.  So the definition, the host twin and the kernel agree BIT FOR BIT on every input, ties
   included: no decision-gap condition is needed.
   BEAM: an ordered list of at most W entries (rank prefix, a, LM state, g, hot-word state, m), at first
   [((), +0.0, start, +0.0, root, 0)].
   POSITION l < n_free: beam entry i in rank order and list rank r < n[l] make candidate index i * K + r with c = ids[l, r]:
     a' = a + val[l, r]; one LM step on c gives g'; one automaton step on c gives m', d';
     key = (a' + s * (m' + d')) + g'       (the hot-word term only with a set that biases, the g term only with a model)
   No candidate is discarded; -inf orders like any other value.  The W best by key stay, ties to the smaller candidate index;
   that order is the new beam's order.  There is no merging: the ids of a list are distinct, so distinct candidates spell
   distinct sequences.
   POSITIONS n_free <= l < L: every entry takes rank 0, a = a + val[l, 0], in order; the LM and the hot words do not see these
   ids (as pf_host_nbest keeps them at the 1-best id).
   FINISH: with PF_LM_EOS and an eos id one eos step without beta; score = (a + s * m) + g_final (the pending part d is
   revoked); re-ordered by descending score, ties to the smaller beam rank; the first N entries are the hypotheses, each with
   ranks [L], score, loglik_sum = a, lm_sum = g_final, matched = m:
     score == (loglik_sum + s * matched) + lm_sum bit for bit.
   NO HYPOTHESES: n_hyp = 0 when L = 0, when some n[l] == 0 for l < L, or when a listed value is NaN or +inf — in the kernel and
   in the twin alike (the twin does not throw here).
   CONSEQUENCES: with no set and alpha = beta = 0 every score is the pf_host_nbest score of that rank vector bit for bit; with
   W >= N the list is pf_host_nbest's list whenever no two hypotheses tie (only the tie rules differ); with W >= K ^ n_free
   nothing is pruned and the list is the brute-force enumeration sorted by score.
   THE MODEL'S OWN </s>: a paraformer emits its </s> id as the last free position and an ARPA file maps </s> to the eos id, so
   that position is already scored as P(</s> | h).  PF_LM_EOS would add a second one: the flag is allowed, leaving it clear is
   recommended.
   OUT OF SCOPE: SeACo (its bias decoder stays the hot-word route), SenseVoice (it has the CTC search), the streaming path,
   pf_group forwards, neural LMs and binary LM formats, merging hypotheses by text. */
/* W = 0 turns the search off; else 1 <= N <= W <= PF_NBEST_MAX (PF_ERR_INVALID_ARG).  Paraformer only: PF_ERR_UNSUPPORTED for
   a SenseVoice or SeACo model.  There is no decode bit of its own (bits 4 and 64 stay invalid): with a search installed a
   forward with PF_DECODE_TOPK runs it right behind the top-k launch, K being pf_engine_set_topk's.  token_ids,
   pf_fetch_scores, pf_fetch_topk and pf_host_nbest are what they are without it.  A pf_group forward over an engine with a
   search installed answers PF_ERR_UNSUPPORTED; the streaming path does not run it. */
int pf_engine_set_nbest_search(pf_engine* e, int32_t W, int32_t N);
/* The model and the hot-word set of the search: argument rules, refusals, the one-time upload and "NULL / 0 clears" are those of
   pf_engine_set_ctc_lm / pf_engine_set_ctc_hotwords, for a paraformer instead of a SenseVoice model.  Inert until a search is
   installed.  (pf_engine_set_ctc_lm, pf_engine_set_ctc_hotwords and PF_DECODE_CTC_BEAM keep refusing a paraformer.) */
int pf_engine_set_nbest_lm(pf_engine* e, const pf_lm* lm, float alpha, float beta, int32_t flags);
int pf_engine_set_nbest_hotwords(pf_engine* e, const int32_t* ids, const int32_t* lens, int32_t n_hotwords, float boost);
/* ranks [B, N, L] int32 (-1 past n_hyp), score / loglik_sum [B, N] float64 (-inf past n_hyp), lm_sum [B, N] float64 (0),
   matched [B, N] int32 (0), n_hyp [B] of the calling thread's last forward, each optional; *L_out and *N_out (optional): the
   L of that forward and the N in force at it.  Slot rules as pf_fetch_ctc_beam (call it BEFORE the pf_fetch that receives
   token_ids).  PF_ERR_INVALID_ARG when that forward ran without a search. */
int pf_fetch_nbest_search(pf_engine* e, int32_t* ranks, double* score, double* loglik_sum, double* lm_sum, int32_t* matched,
                          int32_t* n_hyp, int32_t* L_out, int32_t* N_out);
/* The same search for ONE utterance in plain host code (the twin of the kernel: it runs the same LM step and the same
   automaton table).  hw_* / boost: a hot-word set (n_hotwords == 0 or boost == 0: none; ids in [1, 2^24)); lm (NULL: none)
   with alpha, beta, flags.  out_ranks [N, L], out_score / out_loglik / out_lm [N], out_matched [N] filled as above (all but
   out_ranks optional), *n_hyp.  PF_ERR_INVALID_ARG: bad K / W / N, n[l] outside 0 .. K, a bad boost or weight. */
int pf_host_nbest_search(const int64_t* ids, const float* val, const int32_t* n, int32_t L, int32_t K, int32_t token_num, int32_t W,
                         int32_t N, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords, float boost, const pf_lm* lm,
                         float alpha, float beta, int32_t flags, int32_t* out_ranks, double* out_score, double* out_loglik,
                         double* out_lm, int32_t* out_matched, int32_t* n_hyp);

/* ---- CTC forced alignment (additions to ABI 6; nothing is launched or allocated without the flag) ----------------------
   PF_DECODE_ALIGN (pf_engine_set_decode; SenseVoice only, every math_mode; implies SCORES, not TOPK; independent of
   PF_DECODE_CTC; PF_ERR_UNSUPPORTED for a paraformer or SeACo model and for a pf_group forward): where the text is already
   known — a caller's target, or the hypotheses PF_DECODE_CTC_BEAM keeps — one kernel (csrc/k_ctcalign.hip) behind the other
   decode launches finds the best CTC alignment (Viterbi) of that labeling and the sum over all of its alignments.
   The API takes token IDS: text to ids needs the model's sentencepiece tokenizer and is the caller's business.
   INPUTS per job: the log-prob rows lp[t, :] of the frames t < n_b (the arg-max's in-place rows, prompt rows included, n_b
   as for PF_DECODE_CTC) and a target y[0 .. U) of ids in [1, V); the blank is id 0.  States s in [0, 2U + 1): lab(s) is the
   blank for even s and y[s / 2] for odd s.
   BEST PATH, float32: a[0][0] = lp[0][0], a[0][1] = lp[0][y[0]], else -inf; a[t][s] = best + lp[t][lab(s)] with best among
   the predecessors s, s-1 and (s odd, lab(s) != lab(s-2)) s-2, tried in that order with a strict >: of equal values the
   larger state wins.  The end state is 2U unless a[T-1][2U-1] > a[T-1][2U].  One float add per cell in frame order.
   Per token u: first[u] / last[u] = first / last frame of the path in state 2u+1 (indices in the row, as pf_fetch_ctc),
   tok_score[u] = the largest lp[t][y[u]] of that run.
   LOG-LIKELIHOOD, float64: the same recursion with lse(a, b) = max + log1p(exp(-|a - b|)) (-inf passed through) in place of
   max, ((stay + s-1) + s-2) + lp, ended by lse(a[2U], a[2U-1]): log of the sum over all alignments, which the beam search's
   scores bound from below.
   ok = path_score > -inf.  Not ok (U > n_b, too few frames for repeated ids, n_b = 0 with U > 0, NaN rows; a beam hypothesis
   longer than PF_ALIGN_MAX_TOKENS): first / last hold -1, tok_score 0, path_score / loglik -inf or NaN.  U = 0 is the
   all-blank path; n_b = 0 with U = 0 is ok with score 0.  The definition in numpy is tests/ctcalign_ref.py.
   JOBS of a forward: H = (targets set ? 1 : 0) + (PF_DECODE_CTC_BEAM ? N : 0) per utterance, the caller's target first, then
   the beam's hypotheses in their order (assembled on the device); H = 0 launches nothing.  token_ids, pf_fetch_scores,
   pf_fetch_ctc, pf_fetch_topk and pf_fetch_ctc_beam are what they are without the flag.
   The flag is bit 32; bits 4 and 64 stay unassigned (PF_ERR_INVALID_ARG). */
#define PF_DECODE_ALIGN 32
#define PF_ALIGN_MAX_TOKENS 1023
/* Targets of the NEXT forward on this engine (consumed by it, like the decode lengths): ids [B, cap] int64, len [B] with
   len[b] = -1 for "no target for this row" (its job is skipped).  PF_ERR_INVALID_ARG: PF_DECODE_ALIGN not set, an id outside
   [1, V); PF_ERR_CAPACITY: a len above PF_ALIGN_MAX_TOKENS or cap.  A forward whose batch is not B answers
   PF_ERR_INVALID_ARG before it launches anything (the targets are dropped).  B = 0 clears pending targets. */
int pf_engine_set_align_targets(pf_engine* e, const int64_t* ids, const int32_t* len, int32_t B, int32_t cap);
/* path_score [B, H] fp32, loglik [B, H] float64, ok [B, H], len [B, H] (the job's target length; -1: skipped job, its other
   slots hold -inf / -inf / 0), first / last [B, H, cap] (-1 past len and when not ok), tok_score [B, H, cap] (0 likewise), each
   optional.  *H = jobs per utterance, *len_max = the longest target of the batch.  first / last / tok_score with
   cap < *len_max -> PF_ERR_CAPACITY (H and len_max filled in first).  PF_ERR_INVALID_ARG when that forward ran without the
   flag.  Call it BEFORE the pf_fetch that receives token_ids (it releases the thread's slot). */
int pf_fetch_align(pf_engine* e, float* path_score, double* loglik, int32_t* ok, int32_t* len, int32_t* first, int32_t* last,
                   float* tok_score, int32_t cap, int32_t* H, int32_t* len_max);
/* The same alignment for ONE utterance and ONE target in plain host code (the twin of the kernel): lp [T, ld] (V read per
   row), y [U]; first / last / tok_score [U].  PF_ERR_INVALID_ARG for an id outside [1, V), PF_ERR_CAPACITY for
   U > PF_ALIGN_MAX_TOKENS. */
int pf_host_ctc_align(const float* lp, int64_t ld, int32_t T, int32_t V, const int64_t* y, int32_t U, float* path_score,
                      double* loglik, int32_t* ok, int32_t* first, int32_t* last, float* tok_score);

/* ---- PCM intake (additions to ABI 6) --------------------------------------------------------------------------------
   The audio in the form callers hold it — a wav payload, PCM off a socket — uploaded RAW and turned into the engine's
   float32 mono samples at `fs` by one kernel (csrc/k_pcm.hip) in front of the unchanged fbank.  The result is bit for bit
   what pf_host_wav_read / pf_host_resample produce, i.e. the reference's GetFileSample (Examples/Utils/AudioHelper.cs
   :12-32), quirks included:
     decode    PCM8 b/128-1, PCM16 /32768, PCM24 /8388608, PCM32 /2147483648, float32 unchanged, float64 narrowed,
               G.711 A-law / mu-law expanded to 16-bit first;
     resample  ONLY when sample_rate != fs: stereo is averaged ((l + r) * 0.5f, a trailing unpaired value dropped), then
               linear interpolation in float64, Round(n / ratio) (half to even) output samples (Resample :223-279);
     quirk     at sample_rate == fs nothing is resampled and NOTHING IS DOWN-MIXED: a stereo stream at the native rate
               comes out interleaved, as upstream.  PF_PCM_DOWNMIX_ALWAYS averages the channels at the native rate too.
   n_values counts INTERLEAVED values (data bytes / bytes per value), not frames.
   PF_ERR_INVALID_ARG: data NULL with n_values > 0, channels not 1 or 2, sample_rate <= 0, unknown format, n_values above
   2^31 - 1 (the host definition indexes with int), struct_size mismatch.
   Out of scope: the streaming recognizer's AddSamples (resampling across chunks needs a carried phase the reference's
   one-shot Resample does not define), pf_group_*, more than two channels, compressed containers, sinc / polyphase
   filtering (the reference's linear interpolation is the definition, aliasing included). */
typedef enum pf_pcm_format { PF_PCM_U8 = 1, PF_PCM_S16, PF_PCM_S24, PF_PCM_S32, PF_PCM_F32, PF_PCM_F64, PF_PCM_ALAW, PF_PCM_MULAW } pf_pcm_format;
#define PF_PCM_DOWNMIX_ALWAYS 1
typedef struct pf_pcm_desc { int32_t struct_size, format, sample_rate, channels, flags, reserved[3]; } pf_pcm_desc;
/* Host only: the sample count the conversion yields (to size buffers, or for pf_frontend_num_frames). */
int pf_pcm_num_samples(const pf_pcm_desc* desc, int32_t fs, int64_t n_values, int64_t* n_out);
/* pf_stage_audio for raw PCM: utterance b = n_values[b] values at data[b], described by descs[b] (n_descs == B) or by
   descs[0] (n_descs == 1).  Followed by pf_run_staged / pf_fetch, unchanged. */
int pf_stage_pcm(pf_engine* e, const void* const* data, const int64_t* n_values, const pf_pcm_desc* descs, int32_t n_descs,
                 int32_t B);
/* pf_recognize for raw PCM: hotwords, the per-thread result slot and PF_DECODE_* as there
   (n_b = 4 + pf_frontend_num_frames(pf_pcm_num_samples(...))). */
int pf_recognize_pcm(pf_engine* e, const void* const* data, const int64_t* n_values, const pf_pcm_desc* descs,
                     int32_t n_descs, int32_t B, const int32_t* hotwords, int32_t n_hotwords, pf_batch_out* out);

/* ---- Voice-activity segmentation (additions to ABI 6; nothing is launched or allocated unless one of these is called) ----
   Long audio is cut into utterance-sized pieces on the device: a deterministic, all-integer detector over the 10 ms fbank
   rows the engine already computes (csrc/k_vad.hip).  The per-frame SCORE (step 1) is separate from the state machine
   (steps 2-5): "Voice-activity segmentation, model score" below is its second, learned form.  Every value below is an integer:
   the device form, the host form (pf_host_vad_*) and the definition in numpy (tests/vad_ref.py) agree exactly.
   THE DEFAULT THRESHOLDS ARE STATED, NOT TUNED: nobody has measured them on real speech.
   Frames t = 0 .. T-1 of the whole stream, T = the fbank frame count of n samples; snip_edges = false only
   (PF_ERR_UNSUPPORTED otherwise).
   1 level      per row x[t, 0 .. n_mels) in fp32: v = x; !(v > -64) -> -64 (NaN, -inf); v > 64 -> 64;
                q = (int)rintf(v * 64.f) (half to even); e[t] = sum of q (int32)
   2 threshold  k = min(T - 1, (int64)T * floor_pct / 100); F = the k-th smallest e (0-based);
                thr = max(F + margin_q * n_mels, abs_level) in int64; floor_pct = -1: thr = abs_level; raw[t] = e[t] > thr
   3 hysteresis w = min(window, t + 1), c[t] = raw frames in [t - w + 1, t]; c[t] >= on_count: state[t] = 1; else
                w - c[t] >= off_count: state[t] = 0; else state[t] = state[t - 1] (state[-1] = 0)
   4 padding    d[t] = 1 iff some u in [t - pad_end, t + pad_begin] within [0, T) has state[u] = 1; runs = the maximal [b, e)
                of d; runs with e - b < min_speech are dropped
   5 split      while e - b > max_len: hi = min(b + max_len, e - min_speech), lo = hi - split_search, cut = the t in [lo, hi]
                with the smallest e[t] (ties: the largest t); emit [b, cut), b = cut.  Then emit [b, e).
                Every piece has min_speech <= length <= max_len.
   6 output     [n, 2] int32 frame pairs, ascending.  Segment [b, e) covers the samples [160 b, min(n_samples, 160 e)).
   PF_ERR_INVALID_ARG unless  -1 <= floor_pct <= 100,  1 <= window <= 256,  1 <= on_count, off_count <= window,
   on_count + off_count > window,  0 <= pad_begin, pad_end <= 1024,  min_speech >= 2 * lfr_n (every segment yields an LFR
   frame),  0 <= split_search <= 1024,  2 * min_speech + split_search <= max_len.
   PF_ERR_CAPACITY: T above PF_VAD_MAX_FRAMES, more than PF_VAD_MAX_SEGMENTS segments, or more than the caller's cap
   (the counts are filled in first). */
#define PF_VAD_MAX_SEGMENTS 65536
#define PF_VAD_MAX_FRAMES (1 << 22)
typedef struct pf_vad_config {
  int32_t struct_size;        /* = sizeof(pf_vad_config)                                                   */
  int32_t floor_pct;          /* 10: percentile of the levels taken as the noise floor; -1 = none          */
  int32_t margin_q;           /* 96: speech is this far above the floor, in 1/64 log units per mel bin     */
  int32_t abs_level;          /* INT32_MIN: a lower bound of the threshold                                 */
  int32_t window;             /* 20 frames                                                                 */
  int32_t on_count;           /* 15                                                                        */
  int32_t off_count;          /* 15                                                                        */
  int32_t pad_begin;          /* 30 frames kept in front of speech                                         */
  int32_t pad_end;            /* 5 frames kept behind it                                                   */
  int32_t min_speech;         /* 50                                                                        */
  int32_t max_len;            /* 3000                                                                      */
  int32_t split_search;       /* 500                                                                       */
  int32_t reserved[4];
} pf_vad_config;
/* fills in struct_size and the defaults above */
int pf_vad_default(pf_vad_config* cfg);
/* pf_stage_audio, the ONE batched fbank launch pf_run_staged makes, then the detector's launches over all B utterances;
   only the segment lists are read back.  seg [B, cap, 2] frame pairs, n_seg [B].  cfg == NULL: the defaults. */
int pf_vad_segment(pf_engine* e, const float* const* samples, const int64_t* n_samples, int32_t B, const pf_vad_config* cfg,
                   int32_t* seg, int32_t cap, int32_t* n_seg);
/* The host forms (plain C++, no device): step 1 over rows [T, n_mels]; steps 2-6 over the levels of ONE utterance, lfr_n as
   the engine's front-end has it (seg may be NULL with cap 0 to learn *n). */
int pf_host_vad_levels(const float* rows, int64_t T, int32_t n_mels, int32_t* out);
int pf_host_vad_segments(const int32_t* levels, int32_t T, int32_t n_mels, int32_t lfr_n, const pf_vad_config* cfg, int32_t* seg,
                         int32_t cap, int32_t* n);
/* The batch plan of long-audio recognition (pure host code; part of the definition, because quirk Q2 makes a result depend
   on its batch mates).  len [n]: segment lengths in frames, pooled over the streams of one call.  Order: length descending,
   ties by index ascending.  A batch opens with the longest segment left (length L) and takes the following ones while
   rows < batch_max and (rows + 1) * L <= frame_budget; it always takes at least one.  batch_max <= 0: 32;
   frame_budget <= 0: 96000.  batch [n] / row [n]: where each segment goes; *n_batches (optional). */
int pf_host_long_plan(const int32_t* len, int32_t n, int32_t batch_max, int64_t frame_budget, int32_t* batch, int32_t* row,
                      int32_t* n_batches);

/* ---- Voice-activity endpointing, streaming (additions to ABI 6; nothing is launched or allocated unless one of these is
   called) ----
   The detector above made causal, for audio that is still coming in: it says where a sentence ends while the stream runs
   (csrc/k_endpoint.hip).  The one non-causal step (the percentile floor) is replaced by a tracked floor, the padding step
   becomes events.  Every value past the clamp of step 1 is an integer: the device form, the host form
   (pf_host_endpoint_update) and the definition in numpy (tests/endpoint_ref.py) agree exactly, the state block included.
   THE DEFAULTS ARE STATED, NOT TUNED: there is no speech corpus here, and nobody has measured them on real speech.
   Frames v = 0, 1, ... are the 10 ms fbank rows of the caller's audio; frame v covers the caller's samples from 160 v.
   1  level       e[v]: step 1 above (int32).
   2' floor       F[v] = min(e[v], F[v-1] + rise), F[-1] = +inf (so F[0] = e[0]), in int64: a floor that follows a falling
                  level at once and a rising one at `rise` per frame.  thr[v] = max(F[v] + margin_q * n_mels, abs_level);
                  raw[v] = e[v] > thr[v].  rise = -1: no floor, thr = abs_level.  The floor does not look at the state: one
                  frozen during speech would be a serial feedback loop.  The default rise keeps rise * max_len <
                  margin_q * n_mels (6000 < 7680): a sentence that starts at the floor cannot lose its own speech to the
                  rising floor before the forced cut.
   3  hysteresis  step 3 above word for word (window, on_count, off_count, state[-1] = 0); it is causal as it stands.
   4' events      A state run is a maximal [s0, s1) of state 1.  The first state-1 frame s0 met while no sentence is open opens
                  one at b = max(prev_end, s0 - pad_begin); prev_end is the end of the last emitted sentence, 0 at first.  A
                  run that starts while a sentence is open continues it.  At frame t = s1 - 1 + end_silence, if no state-1
                  frame came in between, the sentence closes with e = s1 + pad_end (pad_end <= end_silence, so e <= t + 1).
                  e - b < min_speech: it is dropped, no event, prev_end does not move.  Otherwise the event
                  (b, e, PF_ENDPOINT_SILENCE) and prev_end = e.
   5' forced cut  after step 4' of frame t, an open sentence with t + 1 - b == max_len gives (b, t + 1, PF_ENDPOINT_FORCED) and
                  prev_end = t + 1.  With state[t] = 1 it stays open (so b = t + 1; its rest falls under min_speech like any
                  sentence), otherwise it is closed.  There is no search for the quietest frame: that would need a level
                  history in the state, and a forced cut is the exception.
   6  flush       the input ends after T frames: an open sentence closes with e = min(T, s1 + pad_end) (T while the state is
                  1), kind PF_ENDPOINT_FLUSH, under the min_speech rule.  Frames after a flush: PF_ERR_INVALID_ARG (a second
                  flush without frames is a no-op).
   7  status      in_speech = a sentence is open; open_begin = its b (-1 when none).
   Event [b, e) covers the samples [160 b, min(n_samples, 160 e)).
   The detector's whole memory between calls is the state block: PF_ENDPOINT_STATE_INTS int32 words, all zero for a fresh stream,
   read and written alike by the host form and the kernel (a stream may change form between any two calls):
     0 .. 7   the raw bits of the previous 256 frames as a 256-bit little-endian number: bit 255 - k is frame count - 1 - k
     8        state of the last frame          9   the last state-1 frame + 1 (0: none)
     10       the first state-1 frame of the open sentence + 1 (0: none open; its b is max(prev_end, that frame - pad_begin))
     11       prev_end                         12  count, the frames seen
     13, 14   F[count - 1] as an int64, low word first (written once count > 0 and rise >= 0)
     15       flushed
   PF_ERR_INVALID_ARG unless  -1 <= rise <= 1 << 20,  the window constraints above,  0 <= pad_begin <= 1024,
   0 <= pad_end <= end_silence <= 1 << 16,  end_silence >= 1 (a run's end shows only at the first state-0 frame),
   min_speech >= 2 * lfr_n,  min_speech <= max_len <= PF_VAD_MAX_FRAMES,  pad_begin < max_len (a sentence is no longer than
   max_len at the frame that opens it); also for a state block no sequence of calls leaves behind (a word outside its range:
   counts and frames in [0, count], flags 0 or 1, the floor inside int32).
   PF_ERR_CAPACITY: count + n_new above PF_ENDPOINT_MAX_STREAM_FRAMES (nothing is changed), or more events than the caller's
   cap: the counts are filled in first, the first cap events are written and the state block HAS advanced. */
#define PF_ENDPOINT_STATE_INTS 16
#define PF_ENDPOINT_MAX_STREAM_FRAMES (1 << 30)
#define PF_ENDPOINT_SILENCE 1
#define PF_ENDPOINT_FORCED 2
#define PF_ENDPOINT_FLUSH 3
typedef struct pf_endpoint_config {
  int32_t struct_size;        /* = sizeof(pf_endpoint_config)                                              */
  int32_t rise;               /* 2: the floor follows a rising level by this much per frame; -1 = no floor */
  int32_t margin_q;           /* 96: speech is this far above the floor, in 1/64 log units per mel bin     */
  int32_t abs_level;          /* INT32_MIN: a lower bound of the threshold                                 */
  int32_t window;             /* 20 frames                                                                 */
  int32_t on_count;           /* 15                                                                        */
  int32_t off_count;          /* 15                                                                        */
  int32_t pad_begin;          /* 30 frames kept in front of speech                                         */
  int32_t pad_end;            /* 5 frames kept behind it                                                   */
  int32_t end_silence;        /* 80 frames without speech end a sentence                                   */
  int32_t min_speech;         /* 50                                                                        */
  int32_t max_len;            /* 3000: the forced cut                                                      */
  int32_t reserved[4];
} pf_endpoint_config;
/* fills in struct_size and the defaults above */
int pf_endpoint_default(pf_endpoint_config* cfg);
/* The host form (plain C++, no device), ONE stream: n_new levels, then the flush if flush != 0.  state
   [PF_ENDPOINT_STATE_INTS] in / out; events [cap, 3] = (b, e, kind) in order, of which the first min(*n_events, cap) rows are
   written (NULL with cap 0 is allowed); lfr_n as the engine's front-end has it; cfg == NULL: the defaults.  in_speech /
   open_begin are optional.  n_new = 0 without a flush changes nothing and reports the status. */
int pf_host_endpoint_update(int32_t* state, const int32_t* levels, int32_t n_new, int32_t flush, int32_t n_mels, int32_t lfr_n,
                            const pf_endpoint_config* cfg, int32_t* events, int32_t cap, int32_t* n_events, int32_t* in_speech,
                            int32_t* open_begin);

/* ---- Voice-activity segmentation, model score (additions to ABI 6; opt-in: with no model attached nothing of this is launched
   or allocated and every result is bit for bit what it is without it) ----
   A second form of step 1: the level of a frame comes from an FSMN-VAD network (the detector FunASR pairs with paraformer and
   SenseVoice) instead of the log-mel energy.  Steps 2-6 are untouched.  The definition in numpy float64 is
   tests/vadnet_ref.py; DESIGN.md 4.6k has the launch plan and the rounding points of the device form (csrc/k_vadnet.hip).
   The model is a `.pfw` of kind "fsmnvad" (python -m aliparaformerasr_amd.convert ... --kind fsmnvad): the dimensions
   input_dim, affine_dim, linear_dim, proj_dim, output_dim, n_layers, lorder, lstride, lfr_m, the silence ids sil_ids and the
   tensors cmvn.shift / cmvn.scale [input], in1 / in2 / out1 / out2 .weight [out, in] and .bias, and per layer l
   fsmn.l.linear.weight [proj, linear], fsmn.l.taps [lorder, proj], fsmn.l.affine.weight [linear, proj] and .bias.
   For frame t of an utterance of T fbank rows x (fp32, n_mels wide; n_mels * lfr_m = input_dim):
     u[t] = concat_j x[clamp(t - (lfr_m - 1) / 2 + j, 0, T - 1)], j = 0 .. lfr_m - 1, then (u + shift) * scale
     a    = ReLU(in2(in1(u)))
     per layer: p = linear(a) (no bias); m[t] = p[t] + sum_k taps[k] * p[t - (lorder - 1 - k) * lstride], rows before the
            utterance's first frame being zeros; a = ReLU(affine(m))
     z    = out2(out1(a));  s = the sum of softmax(z) over sil_ids
     e[t] = rint((1 - 2 s) * 16384), half to even, an int32 in [-16384, 16384]; -16384 where that value is not finite
   The device form multiplies f16 operands with fp32 accumulation (bias, ReLU, the FSMN sum, the softmax and the level in fp32),
   so its levels are close to, not equal to, the host form's; the segments it returns ARE exactly steps 2-6 over its own levels.
   The exact and fp32 math modes of an engine use the same f16 kernel for this network.
   pf_vad_model_config: pf_vad_default with floor_pct = -1 and abs_level = 9830, which is FunASR's rule p_speech >= p_sil + 0.6.
   THESE VALUES ARE AGAIN STATED, NOT TUNED: no threshold has been validated on real speech, and no real FSMN-VAD file has been
   through the converter.
   Loading validates everything.  PF_ERR_INVALID_ARG: not such a container, truncated, a tensor extent outside the file, a
   missing tensor, a wrong shape, a value that is not finite, a silence id outside [0, output_dim).  PF_ERR_UNSUPPORTED:
   rorder > 0, lfr_n != 1, or input / affine / linear / output > 512, proj > 256, n_layers > 8, lfr_m > 16,
   (lorder - 1) * lstride > 256.  PF_ERR_IO: the file cannot be read. */
typedef struct pf_vad_model pf_vad_model;
int pf_vad_model_load(const char* path, pf_vad_model** m);
int pf_vad_model_from_memory(const void* data, int64_t nbytes, pf_vad_model** m);
/* dims [9]: input_dim, affine_dim, linear_dim, proj_dim, output_dim, n_layers, lorder, lstride, lfr_m; each output optional */
int pf_vad_model_info(const pf_vad_model* m, int32_t* dims, int32_t* n_sil, int64_t* image_bytes);
/* sil [cap] (NULL with cap 0 to learn *n); PF_ERR_CAPACITY when cap < *n */
int pf_vad_model_sil_ids(const pf_vad_model* m, int32_t* sil, int32_t cap, int32_t* n);
/* a tensor as loaded, by its container name: out [cap] fp32 (NULL with cap 0 to learn *n); PF_ERR_INVALID_ARG: no such name */
int pf_vad_model_tensor(const pf_vad_model* m, const char* name, float* out, int64_t cap, int64_t* n);
int pf_vad_model_config(pf_vad_config* cfg);
void pf_vad_model_free(pf_vad_model* m);
/* The CPU twins for ONE utterance (plain C++, float64 from the fp32 weights): rows [T, n_mels]; out [T, output_dim] / [T]. */
int pf_host_vad_model_logits(const pf_vad_model* m, const float* rows, int64_t T, int32_t n_mels, double* out);
int pf_host_vad_model_levels(const pf_vad_model* m, const float* rows, int64_t T, int32_t n_mels, int32_t* out);
/* Attaches the model to the engine (NULL detaches and frees what the attach and its runs allocated): pf_vad_segment and everything built on it then compute step 1 with the
   network (profile class "vadnet", 1 + n_layers launches) instead of the energy level (one launch of class "vad").  The engine
   takes a reference of its own (pf_vad_model_free may follow at once) and uploads the weight image once.
   PF_ERR_INVALID_ARG unless n_mels * lfr_m equals the model's input width; PF_ERR_UNSUPPORTED for a snip_edges = true
   front-end.  A pf_group forward is unaffected. */
int pf_engine_set_vad_model(pf_engine* e, const pf_vad_model* m);

/* ---- Voice-activity endpointing, streaming, model score (additions to ABI 6; opt-in: without one of these calls nothing of
   this is launched or allocated and every result is bit for bit what it is without it) ----
   The level of "Voice-activity endpointing, streaming" taken from the FSMN-VAD network of "Voice-activity segmentation, model
   score" instead of the log-mel energy, for B streams per call with each stream's history carried between calls
   (csrc/k_vadnet_stream.hip: ONE launch per call, one workgroup per stream).  The release schedule in Python
   is tests/vadnet_stream_ref.py.
   Let left = (lfr_m - 1) / 2 and right = lfr_m - 1 - left; a stream has received n frames so far.
   The streaming levels (and logits) ARE the levels of "Voice-activity segmentation, model score" over the complete stream,
   released causally; the device form's are bit-equal to the offline device form's, the host form's to the offline host form's.
     - level t is released once frame t + right has arrived, or at the flush;
     - before the flush a stream that has received n frames has released max(0, n - right) levels;
     - the flush releases the rest, and it is the only place where the LFR upper clamp T - 1 applies (T = the frames received);
     - the lower clamp to frame 0 and the zero history in front of frame 0 are the offline definition's: a tap whose source
       lies before frame 0 is skipped, not added as a zero (d <= t on the absolute frame index).
   The endpoint state machine (steps 2' - 7) is unchanged: it sees the released levels in order, so frame indices and times stay
   on the caller's clock.  Because a level waits for `right` later frames, AN EVENT CAN FALL ONE CALL LATER than with the energy
   level.  The decoder-context reset at a sentence end does not reset the network's state: the audio is continuous.
   The state of a stream is opaque, pf_vad_model_stream_state_bytes bytes (a multiple of 16; about 40 KB at the released
   dimensions), all zero for a fresh stream.  It holds per layer the last (lorder - 1) * lstride rows of p in fp32, proj padded to
   32 wide; the last lfr_m - 1 fbank rows received; and in its last 8 bytes the frame count and the flushed flag (int32 each).  The host form has a state of its own
   (float64 history; pf_host_vad_model_stream_state_bytes): a stream cannot change form between calls.
   Frames after a flush: PF_ERR_INVALID_ARG, nothing is launched.  A second flush without frames is a no-op.  n_new = 0 without
   a flush changes no byte of the state.  A count beyond PF_ENDPOINT_MAX_STREAM_FRAMES: PF_ERR_CAPACITY, nothing changed; so is a
   cap below the levels a call releases (at most n_new + right).
   LIMIT: the device form keeps two f16 tiles and a stream's fp32 window in LDS:
     2 * 64 * (widest + 8) * 2 + ((lorder - 1) * lstride + 64) * (round_up(proj_dim, 32) + 4) * 4 <= 159 744 bytes,
   widest = the widest of input_dim (padded to 16), affine_dim, linear_dim, proj_dim (padded to 32).  A model beyond it is
   refused with PF_ERR_UNSUPPORTED by pf_op_vad_model_stream and pf_online_recognizer_set_endpoint_model (the released
   dimensions need 148 272).
   pf_endpoint_model_config: pf_endpoint_default with rise = -1 and abs_level = 9830, the rule pf_vad_model_config states;
   these values are again stated, not tuned. */
int pf_endpoint_model_config(pf_endpoint_config* cfg);
int pf_vad_model_stream_state_bytes(const pf_vad_model* m, int64_t* bytes);
/* The host form (plain C++, float64, the per-row code of pf_host_vad_model_logits), ONE stream: n_new rows [n_new, n_mels], then
   the flush if flush != 0.  state [pf_host_vad_model_stream_state_bytes] in / out; levels [cap] int32 and logits
   [cap, output_dim] float64 (either may be NULL), of which the first *n_out are written. */
int pf_host_vad_model_stream_state_bytes(const pf_vad_model* m, int64_t* bytes);
int pf_host_vad_model_stream(const pf_vad_model* m, void* state, const float* rows, int32_t n_new, int32_t flush, int32_t n_mels,
                             int32_t* levels, double* logits, int32_t cap, int32_t* n_out);

/* ---- Punctuation (additions to ABI 6; opt-in: with no model attached nothing of this is launched or allocated and every
   result is bit for bit what it is without it) ----
   A CT-Transformer (the punctuation model FunASR pairs with paraformer: VAD -> ASR -> punctuation) marks every word of a text
   with one of the model's punctuation classes.  The definition in numpy float64 is tests/punc_ref.py; DESIGN.md 4.6l has the
   launch plan and the rounding points of the device form (csrc/k_punc.hip).  The text rules are THIS PROJECT'S definition,
   restated from FunASR's CTTransformer.inference from memory; the default dimensions are those of FunASR's released
   punc_ct-transformer_zh-cn-common-vocab272727 as remembered.  NO REAL MODEL FILE HAS BEEN LOADED AND NOTHING HERE IS VALIDATED ON ONE.
   The model is a `.pfw` of kind "cttransformer": vocab, d_model, heads, ffn, kernel, n_layers, punc_list (strings),
   sentence_end_id, the u8 tensor "vocab" (the words joined by newlines) and the fp32 tensors embed.weight [vocab, d_model],
   per layer l layers.l.norm1 / attn.qkv / attn.out / norm2 / ffn.w1 / ffn.w2 (.weight [out, in] and .bias),
   layers.l.attn.fsmn.weight [d_model, kernel], after_norm, decoder [n_punc, d_model].
   WORDS: the text is split at ASCII whitespace; inside a piece every character longer than one byte is a word and every
   maximal run of one-byte characters is a word; a word's id is its index in the vocabulary, else that of "<unk>".
   NETWORK, for a window of T <= PF_PUNC_MAX_WINDOW ids: x = fp32(embed[id]) * sqrt(d_model) + pe (positions 1 .. T, [sin || cos]);
   n_layers SAN-M layers (norm1, fused qkv, FSMN over v with `kernel` centred taps inside the window plus identity, softmax
   attention over the window's keys with q scaled by dh^-0.5, out(ctx) + fsmn, residual, norm2, w2(relu(w1)), residual);
   after_norm; decoder; arg-max per row, ties to the larger index.
   TEXT LOOP: the ids are cut into mini-sentences of 20; window m = the carried tail + mini-sentence m.  On the last one the
   whole window is kept and a final "，", "、" or "_" becomes sentence_end_id.  Otherwise the cut is the largest i in
   [2, n - 2] whose mark is "。" or "？"; failing that, when n > 200, the largest i in that range marked "，", which becomes
   sentence_end_id; failing that nothing is emitted (cut = -1).  THE HARD CUT overrules these: when n > 492 and there is no
   cut, or the cut found would leave more than 492 words behind it (n - 1 - cut > 492), the cut is n - 1 and p stays
   unchanged (the comma is then not rewritten).  This is this project's own rule: a carried tail is at most 492 words, so a
   window never passes PF_PUNC_MAX_WINDOW = 492 + 20; FunASR lets it grow.  Words 0 .. cut are emitted, the rest is carried.
   ASSEMBLY: a word is preceded by one space when it and its predecessor both begin with a one-byte character; after such a
   word "，" "。" "？" "、" are written , . ? , and otherwise as listed; "_" and "<unk>" write nothing; no capitalisation.  A
   sentence is a run of words ending at a "。" or "？" (or at the end of the text).
   The device form multiplies f16 operands with fp32 accumulation, so its logits are close to, not equal to, the host form's;
   the loop it runs IS exactly the loop above over its own arg-max.  A window's bits do not depend on its batch mates.
   Loading validates everything.  PF_ERR_INVALID_ARG: not such a container, truncated, a tensor extent outside the file, a
   missing tensor, a wrong shape, a value that is not finite, a vocabulary that is not `vocab` distinct non-empty words or lacks
   "<unk>", a punc_list without "<unk>" / "_", a sentence_end_id outside the list.  PF_ERR_UNSUPPORTED: d_model != 256,
   heads != 8, ffn no multiple of 256 or above 4096, kernel even or above 31, n_layers > 8, fewer than 2 or more than 32
   classes.  PF_ERR_IO: the file cannot be read. */
#define PF_PUNC_MAX_WINDOW 512
#define PF_PUNC_MAX_BATCH 4096
typedef struct pf_punc_model pf_punc_model;
int pf_punc_model_load(const char* path, pf_punc_model** m);
int pf_punc_model_from_memory(const void* data, int64_t nbytes, pf_punc_model** m);
/* dims [16]: vocab, d_model, heads, ffn, kernel, n_layers, n_punc, sentence_end_id, the vocabulary id of "<unk>", then the ids
   of "<unk>" "_" "，" "。" "？" "、" in punc_list (-1: not listed), 0; each output optional */
int pf_punc_model_info(const pf_punc_model* m, int32_t* dims, int64_t* image_bytes);
void pf_punc_model_free(pf_punc_model* m);
/* The CPU twins (plain C++, float64 from the fp32 weights).
   pf_host_punc_words: the words of a text: ids / begin / end [cap] (byte spans in text_utf8; NULL with cap 0 to learn *n);
   PF_ERR_CAPACITY when cap < *n.
   pf_host_punc_logits: ONE window of T ids -> out [T, n_punc].
   pf_host_punc_cut: the cut rule and the last-window edits on one window's p [n] (edited in place) -> *cut.
   pf_host_punc_ids: the text loop over n ids -> punc_ids [n]; win_len / win_cut [win_cap] and *n_win (optional): every
   forward's window length and cut.
   pf_host_punc_assemble: the output text of `text_utf8` (n words, as pf_host_punc_words counts them) under punc_ids [n]: out
   [cap] bytes (no terminator; *out_len is the length needed, PF_ERR_CAPACITY when cap is below it), sent_end [sent_cap] one
   past the last word of each sentence, *n_sent.
   pf_host_punc_text: words, loop and assembly in one call; punc_ids [ids_cap] optional. */
int pf_host_punc_words(const pf_punc_model* m, const char* text_utf8, int32_t* ids, int32_t* begin, int32_t* end, int32_t cap, int32_t* n);
int pf_host_punc_logits(const pf_punc_model* m, const int32_t* ids, int32_t T, double* out);
int pf_host_punc_cut(const pf_punc_model* m, int32_t* p, int32_t n, int32_t last, int32_t* cut);
int pf_host_punc_ids(const pf_punc_model* m, const int32_t* ids, int64_t n, int32_t* punc_ids, int32_t* win_len, int32_t* win_cut,
                     int32_t win_cap, int32_t* n_win);
int pf_host_punc_assemble(const pf_punc_model* m, const char* text_utf8, const int32_t* punc_ids, int32_t n, char* out, int64_t cap,
                          int64_t* out_len, int32_t* sent_end, int32_t sent_cap, int32_t* n_sent);
int pf_host_punc_text(const pf_punc_model* m, const char* text_utf8, char* out, int64_t cap, int64_t* out_len, int32_t* punc_ids,
                      int32_t ids_cap, int32_t* n_words);
/* Attaches the model to the engine (NULL detaches and frees what the attach and its runs allocated).  The engine takes a
   reference of its own (pf_punc_model_free may follow at once) and uploads the weight image once.  Nothing else the engine
   computes changes; a pf_group forward is unaffected. */
int pf_engine_set_punc_model(pf_engine* e, const pf_punc_model* m);
/* The text loop on the device for B texts given as word ids (B <= PF_PUNC_MAX_BATCH): ids = the concatenated ids, lens [B]
   -> punc_ids [sum lens], aligned with ids.  The loop runs in rounds; a round is ONE forward (profile class "punc",
   2 + 2 n_layers launches) over the next window of every text that still has a mini-sentence, and the host only assembles the
   next windows from the cuts.  *rounds (optional): how many rounds ran = the longest text's number of mini-sentences.
   PF_ERR_INVALID_ARG without an attached model or for an id outside the vocabulary. */
int pf_engine_punctuate(pf_engine* e, const int32_t* ids, const int32_t* lens, int32_t B, int32_t* punc_ids, int32_t* rounds);

/* ---- Punctuation, streaming (additions to ABI 6; opt-in: without these calls nothing of it is launched or allocated) ----
   The causal form of the same network punctuates words as they arrive and carries the unfinished sentence between calls
   (FunASR's two-pass runtime does this with its realtime CT-Transformer).  The definition in numpy float64 is
   tests/punc_stream_ref.py; DESIGN.md 4.6s has the state layout, the launch plan and the rounding points of the device form
   (csrc/k_punc_stream.hip: ONE launch per call, one workgroup per stream).  THE DEFINITION IS THIS PROJECT'S; the dimensions of
   FunASR's punc_ct-transformer_zh-cn-common-vad_realtime-vocab272727 are as remembered, its "vad mask" is implied by the
   causal mask in every layer, and whether its last layer is causal is not known here.  NOTHING IS VALIDATED ON A REAL MODEL.
   THE MODEL is a container of kind "cttransformer" whose header adds causal = 1 and sanm_shift (both optional, default 0; a
   container without them loads and behaves bit for bit as before).  The FSMN reach is left = (kernel - 1) / 2 + sanm_shift,
   right = kernel - 1 - left; causal = 1 requires right == 0 and causal = 0 requires sanm_shift == 0, else PF_ERR_UNSUPPORTED.
   pf_host_punc_logits honours both.  The offline device entries (pf_engine_punctuate, pf_op_punc_*,
   pf_recognizer_set_punc_model) refuse a causal model with PF_ERR_UNSUPPORTED, the streaming entries a model that is not.
   THE NETWORK runs on a context w_0 .. w_{n-1}, the words since the last restart: layer-0 input as above with the word's
   index in the context + 1 as its position, attention over the keys j <= i, the FSMN sum
   f_t = v_t + sum_j taps[:, j] v_{t - (kernel - 1) + j} with sources before index 0 skipped, everything else as above.  The
   logits of w_t depend on w_0 .. w_t alone.
   THE LOOP, per stream and per new word in order: the word is appended to the context and its mark is the arg-max of its
   logits, ties to the larger index.  A mark "。" or "？" ends the sentence: the context is emptied behind this word
   (mark_flags bit 0).  Otherwise a context that now holds max_context words (2 .. PF_PUNC_STREAM_MAX_CONTEXT, usually
   PF_PUNC_STREAM_DEFAULT_CONTEXT) is emptied and the mark stays (bit 1: forced restart).  Marks are never revised by later
   words.  THE FLUSH (flush != 0: end of input) edits at most the newest word of the context: *flush_mark is that word's mark,
   with "_", "，" or "、" replaced by sentence_end_id, or -1 for an empty context or without a flush; the context is emptied.
   flags bit 0 (PF_PUNC_STREAM_NO_RESTARTS): the pure network, no rule; a context then holds at most 256 words
   (PF_ERR_INVALID_ARG beyond).
   A stream's state is opaque, pf_punc_stream_state_bytes bytes (f16 keys and values [n_layers, 256, 2, 256] and the count:
   about 1 MB at four layers); all zero is a fresh stream.  The host twin has a state form of its own (float64;
   pf_host_punc_stream_state_bytes).  A word's logits and mark are bit-identical however the stream was cut into calls.
   PF_ERR_INVALID_ARG: max_context or flags out of range, a negative n_new, an id outside the vocabulary, a state whose count
   lies outside its context. */
#define PF_PUNC_STREAM_MAX_CONTEXT 256
#define PF_PUNC_STREAM_DEFAULT_CONTEXT 200
#define PF_PUNC_STREAM_NO_RESTARTS 1
int pf_punc_model_causal(const pf_punc_model* m, int32_t* causal);
int pf_punc_stream_state_bytes(const pf_punc_model* m, int64_t* bytes);
int pf_host_punc_stream_state_bytes(const pf_punc_model* m, int64_t* bytes);
/* COMMITTED WORDS of a streaming recogniser's partial text: the words (as pf_host_punc_words splits them) of the text
   pf_host_online_decode gives for ids; while the last token that contributes text ends in "@@" the last word is held back
   (the next piece changes it).  out [cap]: all the words joined by newlines (no terminator; *out_len the length needed),
   *n_committed of *n_words are committed.  before_utf8 (optional): the committed words of the last call, one per line; they must
   be a prefix of this call's, PF_ERR_RECOGNITION otherwise. */
int pf_host_online_committed_words(const pf_punc_model* m, const char* const* tokens, int32_t n_tokens, const int64_t* ids, int32_t n_ids,
                                   const char* before_utf8, char* out, int64_t cap, int64_t* out_len, int32_t* n_committed, int32_t* n_words);
/* one call of ONE stream in host code, float64: ids [n_new] in order, then the flush.  marks / mark_flags [n_new], logits
   [n_new, n_punc] (optional), *flush_mark (optional) */
int pf_host_punc_stream_step(const pf_punc_model* m, void* state, const int32_t* ids, int32_t n_new, int32_t flush, int32_t max_context,
                             int32_t flags, int32_t* marks, int32_t* mark_flags, double* logits, int32_t* flush_mark);

/* ---- Speaker labels (additions to ABI 6; opt-in: with no model attached nothing of this is launched or allocated and every
   result is bit for bit what it is without it) ----
   Who speaks in each segment of a long recording: a CAM++ network (the speaker model FunASR's AutoModel takes as
   spk_model="cam++") turns windows of fbank rows into embeddings, the cosines of a stream's embeddings are clustered on the
   host, and a segment takes the label most of its windows hold.  The definition in numpy float64 is tests/spk_ref.py;
   DESIGN.md 4.6m has the launch plan and the rounding points of the device form (csrc/k_spk.hip).  The network is stated from
   memory of 3D-Speaker's CAMPPlus (speech_campplus_sv_zh-cn_16k-common, 192-d) and is THIS PROJECT'S definition.  NO REAL
   MODEL FILE HAS BEEN LOADED AND NOTHING HERE IS VALIDATED ON ONE: no dimension, no threshold, and not the front-end (the
   engine's fbank uses a Hamming window, the released model was trained with a Povey window).
   The model is a `.pfw` of kind "campplus": n_mels, m_channels, init_channels, growth, bn_channels, blocks [3], dilations [3],
   seg_len, embedding, and the BatchNorm-folded tensors weights.spk_tensor_shapes lists.
   NETWORK, for a window of T <= PF_SPK_MAX_FRAMES rows x [T, n_mels] of the engine's own fbank: x - mean_t x; the FCM head
   (conv1 3x3, two residual layers of two blocks each, the first of a layer with stride 2 in frequency and a 1x1 shortcut, conv2
   with stride 2 in frequency; ReLU throughout) -> frames of m_channels * n_mels / 8 channels; a TDNN (k 5, stride 2, pad 2, ReLU)
   -> T' = ceil(T / 2) frames; three densely connected blocks of CAM layers (h = ReLU(BN X); b = ReLU(W1 h + c1); a dilated
   k-3 convolution of b times the mask sigmoid(W3 ReLU(W2 c + b2) + b3) of the context c[t] = mean_t b + the mean of b over
   t's segment of seg_len frames; appended to X), each followed by a transit (ReLU(BN), a 1x1 halving the width); ReLU(BN);
   per channel the mean and the unbiased standard deviation over T' (0 when T' = 1); a Linear to `embedding` values, fp32.
   T = 0 gives zeros.  The device form multiplies f16 operands with fp32 accumulation, so its embeddings are close to, not
   equal to, the definition's; a window's bits do not depend on what else is in the call.  Every math mode of an engine uses
   the same f16 kernels for this network.
   WINDOWS of a segment of frames [b, e) under pf_spk_config: none below min_frames; [b, e) up to win; otherwise
   [b + k shift, + win) while they fit, plus [e - win, e) if the last does not end at e.  A stream with more than
   PF_SPK_MAX_WINDOWS windows doubles its shift until it fits.
   CLUSTERING (host, double, deterministic): average linkage over the cosines, cluster similarity updated as
   (nA sAC + nB sBC) / (nA + nB); the pair of largest similarity merges, ties to the smallest first then second index (a
   cluster's index is its earliest window); it stops when the largest similarity is below `threshold`, or, with
   num_speakers > 0, when that many clusters are left (the threshold is then not consulted).  Without num_speakers every cluster
   of fewer than min_cluster windows then joins the cluster of min_cluster or more windows it is most similar to, if there is
   one.  Labels count from 0 in the order of each speaker's first window.  A segment without a window takes the label of the
   labelled segment nearest in time (ties to the earlier), -1 when the stream has none.
   Loading validates everything.  PF_ERR_INVALID_ARG: not such a container, truncated, a tensor extent outside the file, a
   missing tensor, a wrong shape, a value that is not finite.  PF_ERR_UNSUPPORTED: n_mels no multiple of 8 or above 128;
   m_channels no multiple of 8 or above 64; m_channels * n_mels / 8 > 512; init_channels or bn_channels > 128, bn_channels odd;
   growth > 64; a block of more than 64 layers; a dilation > 8; seg_len < 4; a concatenated width that is odd or above 2048;
   embedding > 512.  PF_ERR_IO: the file cannot be read. */
#define PF_SPK_MAX_FRAMES 512
#define PF_SPK_MAX_WINDOWS 8192
typedef struct pf_spk_model pf_spk_model;
int pf_spk_model_load(const char* path, pf_spk_model** m);
int pf_spk_model_from_memory(const void* data, int64_t nbytes, pf_spk_model** m);
/* dims [16]: n_mels, m_channels, init_channels, growth, bn_channels, blocks [3], dilations [3], seg_len, embedding, the frames'
   width, the launches of one forward, 0; each output optional */
int pf_spk_model_info(const pf_spk_model* m, int32_t* dims, int64_t* image_bytes);
void pf_spk_model_free(pf_spk_model* m);
typedef struct pf_spk_config {
  int32_t struct_size;        /* = sizeof(pf_spk_config)                                                   */
  int32_t win;                /* 150 frames per window (1 .. PF_SPK_MAX_FRAMES)                            */
  int32_t shift;              /* 75                                                                        */
  int32_t min_frames;         /* 20: a shorter segment has no window                                       */
  float threshold;            /* 0.5, stated and not tuned                                                 */
  int32_t num_speakers;       /* 0: the threshold decides                                                  */
  int32_t min_cluster;        /* 4                                                                         */
  int32_t reserved[5];
} pf_spk_config;
/* fills in struct_size and the defaults above */
int pf_spk_default(pf_spk_config* cfg);
/* Attaches the model to the engine (NULL detaches and frees what the attach and its runs allocated).  The engine takes a
   reference of its own (pf_spk_model_free may follow at once) and uploads the weight image once.  PF_ERR_INVALID_ARG unless
   the model's n_mels is the engine's.  Nothing else the engine computes changes; a pf_group forward is unaffected. */
int pf_engine_set_spk_model(pf_engine* e, const pf_spk_model* m);
/* The host half (plain C++, no device).  cfg == NULL: the defaults.
   pf_host_spk_windows: the plan of ONE stream: seg [n_seg, 2] frame pairs -> win [cap, 3] (segment, begin, end; NULL with cap
   0 to learn *n; PF_ERR_CAPACITY when cap < *n), *shift_used (optional).
   pf_host_spk_cluster: S [N, N] fp32 (its upper triangle is read; a value that is not finite counts as -2) -> labels [N],
   *n_speakers.
   pf_host_spk_segment_labels: seg [n_seg, 2], the windows' segment and label [N] -> out [n_seg].
   pf_host_spk_centroids: emb [N, E], labels [N] -> out [K, E]: the L2-normalised mean of each speaker's L2-normalised
   embeddings (zeros for a speaker without a window). */
int pf_host_spk_windows(const int32_t* seg, int32_t n_seg, const pf_spk_config* cfg, int32_t* win, int32_t cap, int32_t* n,
                        int32_t* shift_used);
int pf_host_spk_cluster(const float* S, int32_t N, const pf_spk_config* cfg, int32_t* labels, int32_t* n_speakers);
int pf_host_spk_segment_labels(const int32_t* seg, int32_t n_seg, const int32_t* win_seg, const int32_t* win_label, int32_t N,
                               int32_t* out);
int pf_host_spk_centroids(const float* emb, const int32_t* labels, int32_t N, int32_t E, int32_t K, float* out);

/* ------------------------------------------------------------------------ */
/* 4b. Multi-GPU inside one process: one engine, one host thread and one HIP stream per listed
 *     device.  The reference builds a single ORT session (OfflineRecognizer.cs:23); what shards is the utterance
 *     list handed to GetResults (OfflineRecognizer.cs:110-116) — utterances are independent (the batch is dim 0 of
 *     every tensor, OfflineProjOfParaformer.cs:49).  RCCL (dlopen'ed librccl) carries the one-off weight broadcast
 *     devices[0] -> all and the per-call all-gather of the fixed-shape hypotheses; there is no data-path collective.
 *     Every shard is padded to the batch-wide maximum length (PadHelper.cs:25) and decodes the batch-wide maximum
 *     token count, so ids / token_num / cif_peak equal the single-device result position by position.
 *     A device may be listed more than once (several engines on one GPU; no communicator is created then).     */
/* ------------------------------------------------------------------------ */
typedef struct pf_group pf_group;
int pf_group_create(const pf_engine_config* cfg /* .device ignored */, const int32_t* devices, int32_t n_devices,
                    pf_group** out);
void pf_group_destroy(pf_group* g);               /* idempotent, like pf_engine_destroy                       */
int pf_group_info(pf_group* g, int32_t* n_engines, int32_t* uses_rccl);
/* Engine i of the group (borrowed: valid until pf_group_destroy), e.g. for pf_engine_info / profiling.      */
pf_engine* pf_group_engine(pf_group* g, int32_t i);
/* pf_recognize over the whole group: contiguous shards of ceil(B / n_engines) utterances run concurrently, the
   result comes back in the caller's order.  Same two-call protocol as pf_recognize + pf_group_fetch.          */
int pf_group_recognize(pf_group* g, const float* const* samples, const int64_t* n_samples, int32_t B,
                       const int32_t* hotwords, int32_t n_hotwords, pf_batch_out* out);
int pf_group_fetch(pf_group* g, pf_batch_out* out);

/* Host-only rehearsal of pf_group_recognize's control flow (shard plan, the three rendez-vous, the fixed-shape
   all-gather blocks, failure release, merge in the caller's order) with arithmetic stand-ins for the devices, so
   that it runs in a CPU test-suite with G up to 64: utterance u "fires" fire_count[u] tokens and decodes to
   ids[u][l] = u * 100000 + l, token_num[u] = fire_count[u].  has_cif = 0: every non-empty shard reports L = fixed_L
   on its own (SenseVoice).  collective != 0: the hypotheses travel through the all-gather blocks, and shards entering
   the collective with different block sizes — which RCCL answers with a hang — are an error.  fail_shard >= 0: that
   shard throws at fail_stage (0 = in its forward before the decoder-length rendez-vous, 1 = after it, 2 = while
   preparing the gather); the call must then return an error, never hang. */
int pf_host_group_sim(int32_t G, int32_t B, const int32_t* fire_count, int32_t has_cif, int32_t fixed_L,
                      int32_t collective, int32_t fail_shard, int32_t fail_stage, int64_t* ids_out, int32_t l_cap,
                      int32_t* token_num_out, int32_t* L_out);

/* Per-kernel-class device time, measured with HIP events on the engine stream while
   profiling is enabled (bench.py roofline leg).  class_name e.g. "gemm_ffn1". */
int pf_profile_enable(pf_engine* e, int32_t on);
int pf_profile_reset(pf_engine* e);
/* Restrict event recording to one class (NULL or "" = all classes). */
int pf_profile_select(pf_engine* e, const char* class_name);
int pf_profile_get(pf_engine* e, const char* class_name, double* total_ms, int64_t* launches,
                   double* flops_per_launch);
/* GEMM classes: name of the kernel the launcher chose for the class's last profiled launch (the name the
   rocprofv3 kernel trace shows), "" for other classes.  cap = bytes available in name_out. */
int pf_profile_kernel(pf_engine* e, const char* class_name, char* name_out, int32_t cap);

/* Algorithmic FLOPs (2*MAC) of the last forward, SURVEY.md §8(d) formula. */
int pf_last_flops(pf_engine* e, double* flops);

/* ------------------------------------------------------------------------ */
/* 5. Stand-alone device ops exposed for parity tests (tests/ call these through
 *    the C ABI).  pf_op_gemm_ex / pf_op_gemm_rc / pf_op_ffn / pf_op_fsmn_enc / pf_op_fsmn_dec /
 *    pf_op_logsoftmax_argmax / pf_op_attention / pf_op_attention_ex / pf_op_layernorm / pf_op_cif / pf_op_cif_alphas /
 *    pf_op_lfr_cmvn_pad / pf_op_fbank_batch launch exactly the kernels (and kernel variants) the
 *    pipeline launches; pf_op_gemm chooses its variant by shape like the
 *    pipeline does; pf_op_fsmn is a generic fp32 FSMN (arbitrary mask) that the
 *    pipeline itself does not launch; pf_op_argmax scans the values as given. */
/* ------------------------------------------------------------------------ */
/* LFR + CMVN + right-pad + sentinel: fbank rows [t80[b], n_mels] of B utterances -> [B, Tmax, lfr_m*n_mels]. */
int pf_op_lfr_cmvn_pad(pf_engine* e, const float* const* fbank, const int32_t* t80, int32_t B,
                       int32_t apply_sentinel, float* out, int64_t out_cap, int32_t* tmax_out);
/* the batched fbank exactly as pf_run_staged launches it: pf_stage_audio, then ONE fbank launch over all B utterances.
   out = the rows [sum t80, n_mels] of the utterances one after another, t80_out [B] = frames per utterance (filled in
   before PF_ERR_CAPACITY is reported when out_cap floats do not hold the rows). */
int pf_op_fbank_batch(pf_engine* e, const float* const* samples, const int64_t* n_samples, int32_t B, float* out,
                      int64_t out_cap, int32_t* t80_out);
/* last-index arg-max over the trailing dim: x [rows, V] -> ids [rows]. */
int pf_op_argmax(pf_engine* e, const float* x, int64_t rows, int32_t V, int64_t* ids_out);
/* exactly the pipeline's CTC collapse kernel (k_ctc.hip) on caller data: ids / scores [B, T], lens [B] (clamped to
   [0, T]); outputs as pf_fetch_ctc, arrays [B, cap].  PF_ERR_CAPACITY (n_out filled in) when a row has more than cap tokens */
int pf_op_ctc_collapse(pf_engine* e, const int64_t* ids, const float* scores, const int32_t* lens, int32_t B, int32_t T,
                       int32_t blank, int64_t* ids_out, int32_t* first_out, int32_t* last_out, float* score_out, int32_t cap,
                       int32_t* n_out);
/* exactly the pipeline's PCM intake kernel (k_pcm.hip) on caller data: the float samples it hands to the fbank.
   out == NULL: only learn *n_out.  PF_ERR_CAPACITY (n_out filled in) when cap < n_out. */
int pf_op_pcm_convert(pf_engine* e, const void* data, int64_t n_values, const pf_pcm_desc* desc, float* out, int64_t cap,
                      int64_t* n_out);
/* exactly the detector's level kernel (k_vad.hip, step 1 of "Voice-activity segmentation") on caller rows [T, n_mels] fp32:
   out [T] int32.  n_mels: 1 .. 1024. */
int pf_op_vad_levels(pf_engine* e, const float* rows, int64_t T, int32_t n_mels, int32_t* out);
/* exactly the detector's segment kernel (steps 2-6) on caller levels: levels [B, ld] int32 (any values), T [B] frames per
   utterance (0 <= T[b] <= ld), cfg (NULL: the defaults; min_speech is checked against the engine's lfr_n); seg [B, cap, 2],
   n [B].  PF_ERR_CAPACITY (n filled in, the first cap segments of each row stored) when a row has more than cap segments. */
int pf_op_vad_segments(pf_engine* e, const int32_t* levels, const int32_t* T, int32_t B, int32_t ld, int32_t n_mels,
                       const pf_vad_config* cfg, int32_t* seg, int32_t cap, int32_t* n);
/* exactly the streaming endpoint kernel (k_endpoint.hip, steps 2' - 7 of "Voice-activity endpointing, streaming") on caller
   levels, B streams in ONE launch: states [B, PF_ENDPOINT_STATE_INTS] in / out, levels [B, ld] int32 of which stream b's first
   n_new[b] (0 <= n_new[b] <= ld) are its new frames, flush [B] (NULL: none), cfg (NULL: the defaults; min_speech is checked
   against the engine's lfr_n); events [B, cap, 3] of which the first min(n_events[b], cap) rows of a stream are written,
   n_events / in_speech / open_begin [B].  Errors as pf_host_endpoint_update; on an argument error nothing is launched. */
int pf_op_endpoint_update(pf_engine* e, int32_t* states, const int32_t* levels, const int32_t* n_new, const int32_t* flush,
                          int32_t B, int32_t ld, int32_t n_mels, const pf_endpoint_config* cfg, int32_t* events, int32_t cap,
                          int32_t* n_events, int32_t* in_speech, int32_t* open_begin);
/* exactly the attached model's launches (k_vadnet.hip; PF_ERR_INVALID_ARG without pf_engine_set_vad_model) on caller rows: the
   concatenated frames of B utterances, T [B] frames each, rows [sum T, n_mels] fp32; out [sum T, output_dim] fp32 logits /
   out [sum T] int32 levels.  An utterance's result does not depend on its batch mates. */
int pf_op_vad_model_logits(pf_engine* e, const float* rows, const int32_t* T, int32_t B, int32_t n_mels, float* out);
int pf_op_vad_model_levels(pf_engine* e, const float* rows, const int32_t* T, int32_t B, int32_t n_mels, int32_t* out);
/* exactly the attached model's streaming launch (k_vadnet_stream.hip, "Voice-activity endpointing, streaming, model score") on
   caller state blocks and rows, B streams in ONE launch: states [B, pf_vad_model_stream_state_bytes] in / out, rows
   [B, ld, n_mels] of which stream b's first n_new[b] are read, flush [B] (NULL: none); levels [B, cap] int32 and logits
   [B, cap, output_dim] fp32 (either may be NULL) of which stream b's first n_out[b] are written; n_out [B].  Errors as stated
   there; on an argument error nothing is launched and nothing changed. */
int pf_op_vad_model_stream(pf_engine* e, void* states, const float* rows, const int32_t* n_new, const int32_t* flush, int32_t B,
                           int32_t ld, int32_t n_mels, int32_t* levels, float* logits, int32_t cap, int32_t* n_out);
/* exactly the attached punctuation model's launches (k_punc.hip; PF_ERR_INVALID_ARG without pf_engine_set_punc_model) on
   caller windows: the concatenated ids of B windows, T [B] ids each (0 .. PF_PUNC_MAX_WINDOW).
   pf_op_punc_logits: logits [sum T, n_punc] fp32 and, optionally, x0 [sum T, d_model] fp32, the input of layer 0 (1 + 2 n_layers
   launches).  pf_op_punc_window: with the cut launch behind them (2 + 2 n_layers): last [B] != 0 marks a text's last window;
   p [sum T] after the edits, cut [B]; logits optional.  A window's result does not depend on its batch mates. */
int pf_op_punc_logits(pf_engine* e, const int32_t* ids, const int32_t* T, int32_t B, float* logits, float* x0);
int pf_op_punc_window(pf_engine* e, const int32_t* ids, const int32_t* T, const int32_t* last, int32_t B, int32_t* p, int32_t* cut,
                      float* logits);
/* exactly the attached punctuation model's streaming launch (k_punc_stream.hip, "Punctuation, streaming") on caller state
   blocks and ids, B streams (B <= PF_PUNC_MAX_BATCH) in ONE launch (profile class "punc_stream"): states
   [B, pf_punc_stream_state_bytes] in / out, ids [B, ld] of which stream b's first n_new[b] are read, flush [B] (NULL: none);
   marks / mark_flags [B, ld] int32 and logits [B, ld, n_punc] fp32 (logits may be NULL) of which stream b's first n_new[b] are
   written; flush_mark [B].  A stream's result does not depend on its launch mates.  Errors as stated there; on an argument
   error nothing is launched and nothing changed.  A test and tool entry, not the production path: it stages every stream's whole
   state block up and down (about 1 MB each at four layers) and waits twice; pf_online_recognizer_set_punc_model keeps the
   states on the device. */
int pf_op_punc_stream_step(pf_engine* e, void* states, const int32_t* ids, const int32_t* n_new, const int32_t* flush, int32_t B,
                           int32_t ld, int32_t max_context, int32_t flags, int32_t* marks, int32_t* mark_flags, float* logits,
                           int32_t* flush_mark);
/* exactly the attached speaker model's launches (k_spk.hip; PF_ERR_INVALID_ARG without pf_engine_set_spk_model) on caller
   windows: rows = the concatenated fbank rows of B windows, T [B] rows each (0 .. PF_SPK_MAX_FRAMES, else PF_ERR_INVALID_ARG),
   n_mels wide.  emb [B, embedding] fp32; frames (optional) [sum ceil(T / 2), the frames' width] fp32: the activations in front
   of the pooling.  ONE forward (profile class "spk"): 15 launches whatever B and T.  A window's result does not depend on
   what else is in the call.
   pf_op_spk_affinity: emb = the concatenated embeddings of S streams, n [S] each, E wide -> out = the concatenated [n_s, n_s]
   cosine blocks, fp32 in a fixed order of summation (a zero embedding has cosine 0 with everything); one launch of class
   "spk".  Needs no model. */
int pf_op_spk_embed(pf_engine* e, const float* rows, const int32_t* T, int32_t B, int32_t n_mels, float* emb, float* frames);
int pf_op_spk_affinity(pf_engine* e, const float* emb, const int32_t* n, int32_t S, int32_t E, float* out);
/* exactly the pipeline's top-k kernel (k_topk.hip) on the values as given: x [rows, ld] (ld >= V; nothing at or beyond V is
   read in a row), K: 1 .. PF_TOPK_MAX; ids [rows, K], val [rows, K], n [rows] as pf_fetch_topk. */
int pf_op_topk(pf_engine* e, const float* x, int64_t rows, int32_t V, int32_t ld, int32_t K, int64_t* ids, float* val,
               int32_t* n);
/* exactly the pipeline's beam search kernel (k_ctcbeam.hip) on caller arrays: blank_lp [B * T] (dense), ids / val [B * T, K],
   n [B * T], lens [B] (clamped to 0 .. T; nothing at or beyond lens[b] or n[row] is read); outputs as pf_fetch_ctc_beam with
   a token at or beyond cap counted in len but not stored. */
int pf_op_ctc_beam(pf_engine* e, const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens,
                   int32_t B, int32_t T, int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len,
                   double* out_score, int32_t cap, int32_t* n_hyp);
/* the biased form of the same kernel (see "CTC hot words"): pf_op_ctc_beam plus the set, the boost and the two outputs
   [B, N] next to out_score.  boost == 0 or a set without a non-empty word launches exactly what pf_op_ctc_beam launches
   (matched 0, loglik = score). */
int pf_op_ctc_beam_hot(pf_engine* e, const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens,
                       int32_t B, int32_t T, int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len,
                       double* out_score, int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens,
                       int32_t n_hotwords, float boost, int32_t* out_matched, double* out_loglik);
/* the fused forms of the same kernel (see "CTC language model"): pf_op_ctc_beam_hot plus the model, alpha, beta, flags and
   out_lm [B, N].  The image is uploaded into a buffer of its own on first use and kept while the same model is given. */
int pf_op_ctc_beam_lm(pf_engine* e, const float* blank_lp, const int64_t* ids, const float* val, const int32_t* n, const int32_t* lens,
                      int32_t B, int32_t T, int32_t K, int32_t blank, int32_t W, int32_t N, int64_t* out_ids, int32_t* out_len,
                      double* out_score, int32_t cap, int32_t* n_hyp, const int32_t* hw_ids, const int32_t* hw_lens,
                      int32_t n_hotwords, float boost, int32_t* out_matched, double* out_loglik, const pf_lm* lm, float alpha,
                      float beta, int32_t flags, double* out_lm);
/* The n-best search kernel alone on caller-supplied lists for a batch: ids / val [B, L, K], n [B, L], token_num [B]; the
   outputs [B, ...] as pf_fetch_nbest_search fills them (none optional).  The device outputs are sentinel-filled before the
   launch: PF_ERR_DEVICE when a cell comes back unwritten. */
int pf_op_nbest_search(pf_engine* e, const int64_t* ids, const float* val, const int32_t* n, const int32_t* token_num, int32_t B,
                       int32_t L, int32_t K, int32_t W, int32_t N, const int32_t* hw_ids, const int32_t* hw_lens, int32_t n_hotwords,
                       float boost, const pf_lm* lm, float alpha, float beta, int32_t flags, int32_t* out_ranks, double* out_score,
                       double* out_loglik, double* out_lm, int32_t* out_matched, int32_t* n_hyp);
/* lm_walk_kernel (csrc/k_lm.hip), the device twin of pf_host_lm_score: ids [B, L], lens [B] -> g [B, L] float64 and state
   [B, L] after every token p < lens[b]; positions past a length are not written. */
int pf_op_lm_score(pf_engine* e, const pf_lm* lm, const int32_t* ids, const int32_t* lens, int32_t B, int32_t L, float alpha, float beta,
                   double* g, int32_t* state);
/* exactly the pipeline's alignment kernel (k_ctcalign.hip) on caller arrays: lp [B * T, ld] (V read per row), tgt [B, H, cap]
   int32, tlen [B, H] (-1: skip the job; above cap or PF_ALIGN_MAX_TOKENS: ok = 0), lens [B] (clamped to 0 .. T; nothing at or
   beyond lens[b] is read, nor a target slot at or beyond tlen; an id outside [0, V) makes the job not ok).  Outputs as
   pf_fetch_align, every slot written. */
int pf_op_ctc_align(pf_engine* e, const float* lp, int32_t B, int32_t T, int32_t V, int32_t ld, const int32_t* tgt,
                    const int32_t* tlen, const int32_t* lens, int32_t H, int32_t cap, float* path_score, double* loglik,
                    int32_t* ok, int32_t* first, int32_t* last, float* tok_score);
/* C = A[M,K] * W[N,K]^T + bias, f16 operands / f32 accumulate; epilogue 0 none, 1 relu,
   2 = f16 result store (the path the pipeline uses), returned widened to fp32. */
/* One dynamically quantised Linear, the building block of math_mode 2 (the reference's default model.int8.onnx:
   DynamicQuantizeLinear + MatMulInteger + rescale, as onnxruntime's quantize_dynamic emits them for every MatMul with a
   constant weight).  x [M, K] fp32 (x_is_f16: first rounded to f16, as the engine's f16-stored activations are),
   W [N, K] fp32 (quantised per output channel to uint8 here), y [M, N] = float(sum (x_q - x_zp)(w_q - w_zp[n])) *
   (x_scale * w_scale[n]) + bias[n] [ReLU]; the integer sum runs on v_mfma_i32_32x32x32_i8 and is exact.  Optional outputs
   (NULL = skip): the uint8 activations [M, K], {x_scale, x_zp}, the uint8 weights [N, K], w_scale [N], w_zp [N].
   x_is_f16 is a bit set: 1 = round x to f16 first; 2 = run the f16-result kernel of the pipeline's QKV / FFN-up
   projections (y = the stored f16 values widened; PF_ERR_DEVICE if the range its epilogue reports for the next
   quantiser differs from a min / max pass over its output). */
int pf_op_qlinear(pf_engine* e, const float* x, const float* W, const float* bias, int32_t M, int32_t N, int32_t K,
                  int32_t relu, int32_t x_is_f16, float* y, uint8_t* xq_out, float* aparams_out, uint8_t* wq_out,
                  float* wscale_out, int32_t* wzp_out);
/* The parts of the same Linear one at a time, each on a hostile host: whatever the kernels' contracts (csrc/kernels.h) only
   call readable holds a large finite pattern (float vectors behind their last element NaN, the operand pad rows of the GEMM
   the codes +127 / -128, rowsum behind M large magnitudes), every output is sentinel-filled, and PF_ERR_DEVICE is returned
   when a result cell comes back unwritten or anything outside the region the contract allows was stored to.
   pf_op_quantize: DynamicQuantizeLinear of x [rows, cols] fp32 (x_is_f16: handed to the kernels as f16), placed with the row
   stride ldx >= cols on the device, or — gamma / beta [cols] given (ldx == cols, fp32) — of LayerNorm(x) without storing it.
   codes_out [rows, ld]: the signed bytes a' = q - 128 the matrix cores read, pad columns (0) included; rowsum_out [rows] =
   sum_k a'; params_out [2] = {scale, zero point}. */
int pf_op_quantize(pf_engine* e, const float* x, int32_t rows, int32_t cols, int32_t ldx, int32_t x_is_f16, int32_t ld,
                   const float* gamma, const float* beta, int8_t* codes_out, int32_t* rowsum_out, float* params_out);
/* The weight side: W [N, K] fp32 quantised per output channel (pf_op_quantize_weight), or the stored bytes of an int8 export
   Q [N, K] u8, zp [N] u8, scale [N] (pf_op_import_weight) -> w_out [N, ld] signed bytes w' = q - 128 (pad columns 0),
   colsum_out [N] = sum_k w', wzp_out [N] = zp - 128, wscale_out [N], dz_out [N] the packed column word of the f16-result
   kernel (PF_ERR_UNSUPPORTED when K > 16384: the word does not hold it). */
int pf_op_quantize_weight(pf_engine* e, const float* W, int32_t N, int32_t K, int32_t ld, int8_t* w_out, int32_t* colsum_out,
                          int32_t* wzp_out, float* wscale_out, int32_t* dz_out);
int pf_op_import_weight(pf_engine* e, const uint8_t* Q, const uint8_t* zp, const float* scale, int32_t N, int32_t K, int32_t ld,
                        int8_t* w_out, int32_t* colsum_out, int32_t* wzp_out, float* wscale_out, int32_t* dz_out);
/* The integer GEMM alone, on codes and parameters as given (no quantiser runs): the operands a', w', the row / column sums
   and dz are built on the host. */
typedef struct pf_qgemm_desc {
  int32_t struct_size;
  int32_t M, N, K;            /* K = the true depth (the operands are padded to a multiple of 128 with zeros)            */
  int32_t relu;
  int32_t out_kind;           /* 0 fp32 (resid, when given, aliases the result), 1 f16 into a padded buffer with dz
                                 (gemm_i8f_pp3), 2 f16 unpadded (gemm_i8_pp3's direct epilogue), 3 fp32 and f16 together  */
  int32_t tile_rows;          /* 0 = by shape, 128 / 256 = the tile height                                              */
  int32_t want_range;         /* != 0: the launch reports the {min, max} of its results (range_out)                     */
  int32_t scale_cols;         /* columns n < scale_cols are multiplied by scale after the bias                          */
  float scale;
  float a_scale; int32_t a_zp;   /* the activation tensor's parameters, zero point in 0 .. 255                         */
  const int32_t* w_zp;        /* [N], 0 .. 255                                                                          */
  const float* w_scale;       /* [N]                                                                                    */
  const float* bias;          /* [N] or NULL                                                                            */
  const float* resid;         /* [M,N] fp32 or NULL (out_kind 0, 2, 3)                                                  */
  const float* add2;          /* [M,N] fp32 or NULL (out_kind 0, 2, 3)                                                  */
} pf_qgemm_desc;
/* a_codes [M, K], w_codes [N, K] uint8; y32 [M, N] (out_kind 0, 3), y16 [M, N] widened to fp32 (out_kind 1, 2, 3),
   range_out [2] (want_range); the kernel's name is left under the profile class "gemm_op" (pf_profile_kernel). */
int pf_op_qgemm_ex(pf_engine* e, const pf_qgemm_desc* d, const uint8_t* a_codes, const uint8_t* w_codes, float* y32, float* y16,
                   float* range_out);
int pf_op_gemm(pf_engine* e, const float* A, const float* W, const float* bias,
               int32_t M, int32_t N, int32_t K, int32_t epilogue, float* C);
/* The GEMM as the pipeline launches it, every variant selectable. */
typedef struct pf_gemm_desc {
  int32_t struct_size;
  int32_t M, N, K;
  int32_t relu;
  int32_t out_kind;           /* 0 fp32 result (+ residual / addend), 1 f16 row-major, 2 f16 blocked layout
                                 (32 rows x 8 columns = 512 contiguous bytes; the encoder FFN hidden)         */
  int32_t a_blocked;          /* A is handed to the kernel in the blocked layout (FFN-down's operand)         */
  int32_t tile_rows;          /* kernel selector: 0 = by shape as the pipeline does (M <= 512 rows: the short-input
                                 kernel; blocked results with fewer idle rounds: the persistent 256 x 256 kernel);
                                 128 / 256 = gemm_f16_pp3 tile heights; 512 = the 256 x {192,256} tile kernel, one tile
                                 per workgroup; 1024 = its persistent form (blocked result only); 32 = the short-input
                                 kernel; 2048 = the k-step-32 six-stage kernel (fp32 results of deep-K projections, the
                                 encoder's FFN-down).  PF_ERR_INVALID_ARG when the named kernel does not apply.     */
  int32_t scale_cols;         /* columns n < scale_cols are multiplied by scale after the bias (q scaling)    */
  float scale;
  const float* bias;          /* [N] or NULL                                                                  */
  const float* resid;         /* [M,N] fp32 or NULL (out_kind 0)                                              */
  const float* add2;          /* [M,N] fp32 or NULL (out_kind 0): the FSMN memory added by the out-projection */
} pf_gemm_desc;
/* C [M,N] fp32 (f16 results widened, blocked results de-blocked on the host). */
int pf_op_gemm_ex(pf_engine* e, const pf_gemm_desc* d, const float* A, const float* W, float* C);
/* The K = 512 product C [M,N] = A [M,512] W [N,512]^T + bias (bias may be NULL) as the decoder's K | V projection and the
   vocabulary layer launch it.  form: 7 = the panel-resident kernel, 1 / 2 = gemm_f16_pp3 with 128- / 256-row tiles, 0 = by the
   pipeline's rule.  out_kind: 0 = fp32 result (row stride round_up(N, 4)), 1 = f16 result (row stride N + 64; N % 4 == 0),
   widened into C.  padded != 0 declares the result rows up to round_up(M, 256) writable, as the pipeline's buffers are.  The
   operand rows behind M - 1 / N - 1 hold NaNs and the result buffer is guarded: PF_ERR_DEVICE when a cell of [M, N] was
   not written or any other cell was.                                                                                 */
int pf_op_gemm_panel(pf_engine* e, int32_t M, int32_t N, int32_t out_kind, int32_t form, int32_t padded, const float* bias,
                     const float* A, const float* W, float* C);
/* Row-complete GEMM (N = 512) with its fused epilogue, as the encoder launches it for the attention output
   projection and the FFN down-projection: x = resid + A W^T + bias + FSMN_k(v) ; n = LayerNorm(x). */
typedef struct pf_gemm_rc_desc {
  int32_t struct_size;
  int32_t M, K;
  int32_t a_blocked;          /* A handed over in the blocked activation layout                                */
  int32_t T;                  /* utterance length in rows (FSMN zero padding at utterance edges); 0 = M        */
  int32_t fsmn_k;             /* taps of fsmn_w (11), 0 = no FSMN term                                          */
  const float* bias;          /* [512] or NULL                                                                 */
  const float* resid;         /* [M,512] or NULL                                                               */
  const float* fsmn_v;        /* [M,512] (rounded to f16 on the device, as the V slice is) or NULL             */
  const float* fsmn_w;        /* [512, fsmn_k]                                                                 */
  const float* ln_gamma;      /* [512] or NULL (no LayerNorm outputs)                                          */
  const float* ln_beta;
  int32_t short_input;        /* 1 = the kernels the pipeline uses for M <= 512 rows (k_gemm_small.hip): K <= 576:
                                 one-shot GEMM with the FSMN memory as an epilogue term, then the LayerNorm kernel;
                                 K > 576: split partials + the reduction that carries the LayerNorm (no FSMN term) */
  int32_t split_k;            /* must be 0: the split-K forms of round 4 (k_gemm_sk.hip) lost to the fused FFN block and
                                 were removed in round 5 (PF_ERR_UNSUPPORTED); the field keeps the struct layout     */
} pf_gemm_rc_desc;
/* x_out [M,512] fp32 (may be NULL), n16_out [M,512] (the f16 LayerNorm result widened to fp32, may be NULL),
   n32_out [M,512] fp32 LayerNorm result (may be NULL). */
int pf_op_gemm_rc(pf_engine* e, const pf_gemm_rc_desc* d, const float* A, const float* W, float* x_out,
                  float* n16_out, float* n32_out);
/* Encoder FFN with the blocked hand-off of the hidden: y = resid + W2 relu(W1 x + b1) + b2;
   x [M,D], w1 [F,D], w2 [D,F], resid / y [M,D]. */
int pf_op_ffn(pf_engine* e, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
              const float* resid, int32_t M, int32_t D, int32_t F, float* y);
/* The same block as the pipeline launches it for long inputs since round 5 (k_ffn.hip, ONE launch, the hidden stays in
   LDS; d_model 512, hidden 2048): x_out = resid + W2 relu(W1 x + b1) + b2 [M,512] (may be NULL), n16_out = the f16
   LayerNorm(x_out; gamma, beta) widened to fp32 (NULL, or with gamma / beta).  resid may be NULL (zeros). */
int pf_op_ffn_fused(pf_engine* e, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                    const float* resid, const float* ln_gamma, const float* ln_beta, int32_t M, float* x_out, float* n16_out);
/* The decoder's position-wise block as the pipeline runs it since round 5 (k_ffn.hip, split form; d_model 512, hidden 2048):
   t = LayerNorm_F(relu(x w1^T + b1); gamma_f, beta_f) w2^T  (the w_1 / norm / w_2 nodes of a decoder layer, w2 without bias),
   n = LayerNorm(t; ln_gamma, ln_beta).  x [M,512] = the block's normalised input (rounded to f16 like every f16-mode operand) —
   or, with ctx != NULL, the PREVIOUS layer's cross-attention out-projection runs in front of the block in the same launch:
   x_out = resid + ctx wo^T + bo, the block's input = LayerNorm(x_out; ln1_gamma, ln1_beta) (x is then ignored).
   splits: how many workgroups share a 64-row tile's hidden range, 0 = the pipeline's choice for M, or 1 | 2 | 3 | 4 | 8. */
typedef struct pf_dec_ffn_desc {
  int32_t struct_size;           /* sizeof(pf_dec_ffn_desc) */
  int32_t M, splits, reserved;   /* reserved = 0 */
  const float* x;                /* [M,512] or NULL with ctx */
  const float* w1; const float* b1;            /* [2048,512], [2048] */
  const float* gamma_f; const float* beta_f;   /* [2048] */
  const float* w2;                             /* [512,2048] */
  const float* ln_gamma; const float* ln_beta; /* [512] or NULL */
  const float* ctx; const float* wo; const float* bo; const float* resid;   /* [M,512], [512,512], [512], [M,512] or all NULL */
  const float* ln1_gamma; const float* ln1_beta;                           /* [512], with ctx */
} pf_dec_ffn_desc;
/* t_out / n_out / x_out [M,512] fp32, each may be NULL (n_out needs ln_gamma / ln_beta, x_out needs ctx). */
int pf_op_dec_ffn_fused(pf_engine* e, const pf_dec_ffn_desc* d, float* t_out, float* n_out, float* x_out);
/* The middle of a decoder layer on caller data, in the three forms the engine can run it (d_model 512, hidden 2048, M = B L):
     t  = LayerNorm_F(relu(a w1^T + b1); gamma_f, beta_f) w2^T          the position-wise block of pf_op_dec_ffn_fused, split form
     tn = LayerNorm(t; n2), a zero row at the positions l >= token_num[b]
     x += sum_j taps[j] tn[l + j - 5] + tn[l]      for l < token_num[b]   (11 taps [11][512]; a masked row of x keeps its bits)
     xn = f16 LayerNorm(x; n3)                     on every row
     q  = f16((xn wq^T + bq) / sqrt(128))
   form 0: the split launch without its finishing pass + ONE launch of the fused kernel (k_decmid.hip);
   form 1: the split launch with its finishing pass and norm2, the fused FSMN + norm3 kernel, the q GEMM;
   form 2: the same with the FSMN kernel and the LayerNorm kernel as two launches.
   x_out [M,512] fp32, q_out [M,512] (the stored f16 widened to fp32); tn_out (fp32) and xn16_out (f16 widened) exist in forms
   1 and 2 only and may be NULL.  *ran = 1 when the form ran as asked, 0 when form 0 declined the geometry (nothing is returned
   then).  In form 0 the workspace rows of the masked positions are overwritten with a large finite pattern between the two
   launches.  q is stored with a row stride of 520 halves; the 8 columns behind it, the rows of x and q behind M - 1 and, in
   form 0, the bits of every masked row of x are checked after the launch (PF_ERR_DEVICE names the cell). */
typedef struct pf_dec_mid_desc {
  int32_t struct_size;           /* sizeof(pf_dec_mid_desc) */
  int32_t B, L, splits, form, reserved;   /* splits as pf_dec_ffn_desc; reserved = 0 */
  const float* a;                /* [M,512] the block's normalised input */
  const float* w1; const float* b1;            /* [2048,512], [2048] */
  const float* gamma_f; const float* beta_f;   /* [2048] */
  const float* w2;                             /* [512,2048] */
  const float* n2_gamma; const float* n2_beta; /* [512] */
  const float* taps;                           /* [11][512] */
  const int32_t* token_num;                    /* [B], 0 <= token_num[b]; values above L count as L */
  const float* x;                              /* [M,512] the residual stream */
  const float* n3_gamma; const float* n3_beta; /* [512] */
  const float* wq; const float* bq;            /* [512,512], [512] */
} pf_dec_mid_desc;
int pf_op_dec_mid(pf_engine* e, const pf_dec_mid_desc* d, float* x_out, float* q_out, float* tn_out, float* xn16_out, int32_t* ran);
/* The fused decoder FSMN + LayerNorm kernel (k_norm.hip) alone: x_out = x + (sum_j taps[j] tn[l + j - (k - 1) / 2] + tn[l]) for
   l < token_num[b] (taps [k][512], k = 11 | 21; tn, x [B L,512]), xn16_out = f16 LayerNorm(x_out; gamma, beta) of every row.  The
   rows of tn at l >= token_num[b] are replaced by a large finite pattern on the device: they must not reach any result. */
int pf_op_fsmn_dec_ln(pf_engine* e, const float* tn, const float* taps, const int32_t* token_num, int32_t B, int32_t L, int32_t k,
                      const float* x, const float* gamma, const float* beta, float* x_out, float* xn16_out);
/* The row kernels of k_norm.hip and of the non-CIF half of k_misc.hip, each launcher alone on caller data (tests/rows_ref.py).
   Every result buffer below is GUARDED: a result of R rows with row stride ld comes back as (R + 2 PF_OP_GUARD_ROWS) rows of ld
   cells, the result in rows [PF_OP_GUARD_ROWS, PF_OP_GUARD_ROWS + R).  Before the launch every cell holds the canary
   (PF_OP_CANARY32 in 32-bit cells, twice in 64-bit cells, PF_OP_CANARY16 in f16 cells); the buffer is returned whole and nothing
   is checked on the way: what was written outside the result is the caller's to judge.  f16 data travels as bit patterns. */
#define PF_OP_GUARD_ROWS 2
#define PF_OP_CANARY32 0x7FC5A5A5u
#define PF_OP_CANARY16 0x7E5Au
/* launch_layernorm: x [rows,D] (D % 4 == 0, D <= 2048; two rows of a large finite pattern lie behind it on the device) ->
   out16 guarded [rows, ld16] f16 and / or out32 guarded [rows, ld32] fp32 (either may be NULL; ld % 4 == 0, ld >= D).
   posenc_T > 0: launch_posenc_ln_tab instead, x = [rows / posenc_T, posenc_T, D] with D the model's feature width, scaled by
   sqrt(d_model) and position-encoded from the engine's own table (built as the encoder builds it); f16 result only. */
int pf_op_layernorm_ex(pf_engine* e, const float* x, const float* gamma, const float* beta, int64_t rows, int32_t D, int32_t ld16,
                       int32_t ld32, int32_t posenc_T, uint16_t* out16, float* out32);
/* launch_layernorm_f16: x [rows,D] f16 (D % 8 == 0, D <= 2048) -> out guarded [rows, D] f16; in_place != 0: x is placed in the
   result buffer itself and normalised there, as the decoder does with its FFN hidden. */
int pf_op_layernorm_f16(pf_engine* e, const uint16_t* x, const float* gamma, const float* beta, int64_t rows, int32_t D, int32_t in_place,
                        uint16_t* out);
/* launch_fsmn_dec_stream: the decoder FSMN of the streaming graph over xc = [cache_in | tn * m], m = (l < len[b]):
     x[b,l,:] += sum_j taps[j] xc[l + j] + tn[l]   for l < len[b];   cache_out = the last k - 1 columns of xc.
   tn, x [B,L,D]; taps [k,D]; cache_in [B,D,k-1]; len [B] (a value above L counts as L).  x_out guarded [B L, D], cache_out
   guarded [B D, k-1].  The rows of tn at l >= len[b] are replaced by a large finite pattern on the device. */
int pf_op_fsmn_dec_stream(pf_engine* e, const float* tn, const float* taps, const int32_t* len, const float* cache_in, int32_t B, int32_t L,
                          int32_t D, int32_t k, const float* x, float* x_out, float* cache_out);
/* The stand-alone FSMN memory blocks of k_misc.hip, each launcher alone (tests/fsmn_ref.py):
     y[b,t,:] = m_t ((v m)[b,t,:] + sum_j taps[j] (v m)[b, t + j - (k - 1) / 2, :]),   zero outside [0, T);   taps [k,D].
   On the device the operand lies in a buffer of B T + 16 rows of ldv cells that holds a large finite pattern everywhere outside
   the V columns [col, col + D) of rows [0, B T); the result comes back guarded, [B T, D].  The kernel that ran is read with
   pf_profile_kernel(e, "gemm_op") (profiling on).
   launch_fsmn_enc: v16 [B T, D] as f16 bit patterns, no mask; k outside {3, 5, 7, 9, 11}, a D that is no multiple of 4 or an
   ldv / col that is none is refused by the launcher (PF_ERR_UNSUPPORTED). */
int pf_op_fsmn_enc_ex(pf_engine* e, const uint16_t* v16, const float* taps, int32_t B, int32_t T, int32_t D, int32_t k, int32_t ldv,
                      int32_t col, float* y_out);
/* launch_fsmn_f32 / launch_fsmn_f32_ld: v [B T, D] fp32, mask [B,T] floats (NULL: none; it multiplies, fractions allowed).
   form 0: what the pipeline launches — launch_fsmn_f32 on dense rows (ldv == D, col == 0), launch_fsmn_f32_ld on strided ones
   (no mask, k = 11);  1: launch_fsmn_f32 with the generic kernel forced (dense, no mask);  2: launch_fsmn_f32 with its result on
   its operand, which the launcher refuses (PF_ERR_INVALID_ARG) before anything runs. */
int pf_op_fsmn_f32_ex(pf_engine* e, const float* v, const float* taps, const float* mask, int32_t B, int32_t T, int32_t D, int32_t k,
                      int32_t ldv, int32_t col, int32_t form, float* y_out);
/* launch_fsmn_dec: x_out guarded [B L, D] = x + y with m = (l < token_num[b]), any k.  The rows of tn at l >= token_num[b] are
   replaced on the device by `hostile`: 0 a large finite pattern, 1 NaN, 2 +-Inf; a row of x at l >= token_num[b] must come back
   with the bits it went in with (PF_ERR_DEVICE otherwise). */
int pf_op_fsmn_dec_ex(pf_engine* e, const float* tn, const float* taps, const int32_t* token_num, int32_t B, int32_t L, int32_t D,
                      int32_t k, int32_t hostile, const float* x, float* x_out);
/* launch_embed_gather: out32 guarded [rows, D] = table[clamp(ids[r], 0, vocab - 1)], out16 (may be NULL) its f16 rounding.  On the
   device the table lies between two rows of a large finite pattern. */
int pf_op_embed_gather(pf_engine* e, const float* table, const int32_t* ids, int32_t rows, int32_t D, int32_t vocab, float* out32,
                       uint16_t* out16);
/* launch_add_to_f16: out16 guarded [rows, D] = f16(a + b), the sum rounded to fp32 first. */
int pf_op_add_to_f16(pf_engine* e, const float* a, const float* b, int64_t rows, int32_t D, uint16_t* out16);
/* launch_seaco_merge: row r is REPLACED iff the first-index arg-max of dha[r, :V] is not nobias, or dha[r, nobias] is NaN, or nobias
   lies outside [0, V): then ids[r] = dha_ids[r] and, with copy_logits, logits[r, :V] = dha[r, :V].  dha [rows, ld_dha] goes up with
   its pad columns as given; logits_in [rows, ld_logits] and ids_in [rows] are what the buffers hold before the launch;
   logits_out guarded [rows, ld_logits], ids_out guarded [rows] (int64). */
int pf_op_seaco_merge(pf_engine* e, const float* dha, int32_t ld_dha, const int64_t* dha_ids, int64_t rows, int32_t V, int32_t nobias,
                      int32_t copy_logits, const float* logits_in, int32_t ld_logits, const int64_t* ids_in, float* logits_out,
                      int64_t* ids_out);
/* *rows = the row count up to which this engine's encoder takes its short-input kernels (k_gemm_small.hip); 0: never. */
int pf_op_short_input_max_rows(pf_engine* e, int32_t* rows);
/* The same launch with the attention out-projection in front of the block, as the pipeline runs two thirds of an encoder
   layer since round 5: x_mid = resid + ctx wo^T + bo + FSMN(v) (11 taps, utterances = runs of T rows);
   x_out = x_mid + W2 relu(W1 LayerNorm(x_mid; ln2) + b1) + b2; n16_out = f16 LayerNorm(x_out; ln_gamma, ln_beta).
   ctx, v [M,512]; wo [512,512]; fsmn_w [512,11]; resid may be NULL. */
typedef struct pf_attn_ffn_desc {
  int32_t struct_size; int32_t M; int32_t T; int32_t reserved;
  const float* ctx; const float* wo; const float* bo; const float* v; const float* fsmn_w;
  const float* ln2_gamma; const float* ln2_beta; const float* resid;
  const float* w1; const float* b1; const float* w2; const float* b2;
  const float* ln_gamma; const float* ln_beta;
  /* optional tail, as the pipeline runs it between two encoder layers: the NEXT layer's fused Q | K | V projection of
     LayerNorm(x_out; ln_gamma, ln_beta) in the same launch: wqkv [1536,512] = [Q | K | V] rows, bqkv [1536]; q_out (scaled by
     1/sqrt(128)), k_out, v_out [M,512] = the stored f16 values widened to fp32 (each may be NULL) */
  const float* wqkv; const float* bqkv; float* q_out; float* k_out; float* v_out;
} pf_attn_ffn_desc;
int pf_op_attn_ffn_fused(pf_engine* e, const pf_attn_ffn_desc* d, float* x_out, float* n16_out);
/* A Linear of the fp32 graph as the engine's math_mode runs it (engines created with math_mode 1 or 3 only):
     y [M,N] = x [M,K] W[N,K]^T + bias [+ resid [M,N]] [ReLU]
   math_mode 3 ("exact"): operands as (hi, lo') f16 pairs, the three partial products in ONE accumulation of the pipeline's
   f16 MFMA kernel (K-loop wrap, csrc/kernels.h) — the stand-alone counterpart of Engine::gemm32.  bias / resid may be NULL. */
int pf_op_linear32(pf_engine* e, const float* x, const float* W, const float* bias, const float* resid, int32_t M, int32_t N,
                   int32_t K, int32_t relu, float* y);
/* The FFN block of the fp32 graph as math_mode 1 / 3 runs it: y [M,D] = x + relu(x W1^T + b1) W2^T + b2, W1 [F,D], W2 [D,F].
   In math_mode 3 above the short-input threshold the hidden never exists in fp32: the first product's epilogue writes it as
   the (hi, lo') operand pair of the second (what the encoder layers do). */
int pf_op_ffn32(pf_engine* e, const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int32_t M,
                int32_t D, int32_t F, float* y);
/* The same Linear on a hostile host, every argument of Engine::gemm32 selectable: A [M,K] and W [N,K] are placed with the row
   strides lda / ldw (0 = K), the result with ldc (0 = round_up(N, 4)), the residual with ldr (0 = ldc) or, resid_aliases_out != 0,
   in the result buffer itself (what the layers do with the residual stream); resid2 is gemm32's second addend (row stride
   ldr).  Whatever lies outside the matrices holds a large finite pattern, the x3 arenas are filled with one before the call,
   and the result buffer is checked for unwritten cells of [M,N] and for stores outside it.  flags: gemm32's (1 = result as an
   operand pair, 2 = operand is that pair, 4 = same operand as the previous call).  The kernels that ran are read with
   pf_profile_kernel: class "gemm32_op" (math_mode 3, two-launch form: the second launch; the first is "gemm32_x3_main"). */
typedef struct pf_linear32_desc {
  int32_t struct_size;
  int32_t M, N, K;
  int32_t lda, ldw, ldc, ldr;
  int32_t resid_aliases_out;
  int32_t relu;
  int32_t scale_cols;         /* columns n < scale_cols are multiplied by scale (after the bias); 0 = none */
  float scale;
  int32_t flags;
  const float* bias;          /* [N] or NULL   */
  const float* resid;         /* [M,N] or NULL */
  const float* resid2;        /* [M,N] or NULL */
} pf_linear32_desc;
int pf_op_linear32_ex(pf_engine* e, const pf_linear32_desc* d, const float* A, const float* W, float* C);
/* split_x3_kernel alone: x [rows,K] (placed with row stride ldx >= K) -> out [rows, ldo] f16 bit patterns, hi at columns
   [0, Kp), lo' at [Kp, 2 Kp) (swap != 0: the other way round); the buffer is pre-filled with 0x7E5A and checked for stores
   behind row rows - 1.  Domain: finite |x| < 65520. */
int pf_op_split_x3(pf_engine* e, const float* x, int32_t rows, int32_t K, int32_t ldx, int32_t ldo, int32_t Kp, int32_t swap, uint16_t* out);
/* LayerNorm of the fp32 graph (Engine::layernorm32): x [M,D] -> out32 [M,D], or, where math_mode 3 writes the operand pair
   instead (D = 512, M above the short-input threshold), pair [M, 2 D] = hi | lo' f16 bit patterns and *wrote_pair = 1 (out32 is
   then left alone).  direct_pair != 0: launch_layernorm_pair itself at any M (D = 512).  W [N,D] != NULL: followed by the
   consuming gemm32, y [M,N] = LayerNorm(x) W^T + bias — the hand-over through the arena as the encoder layers do it. */
int pf_op_layernorm32(pf_engine* e, const float* x, const float* gamma, const float* beta, int32_t M, int32_t D, int32_t direct_pair,
                      float* out32, uint16_t* pair, int32_t* wrote_pair, const float* W, const float* bias, int32_t N, float* y);
/* pf_op_ffn32 on a hostile host with the hidden scaled by hidden_scale (1 = no scale) before the ReLU:
   y = x + relu((x W1^T + b1) s) W2^T + b2.  Where the hidden travels as an operand pair, hidden_pair [M, 2 F] receives its
   hi | lo' bit patterns and *pair_written = 1.  Profile classes "gemm32_ffn1" and "gemm32_ffn2". */
int pf_op_ffn32_ex(pf_engine* e, const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int32_t M,
                   int32_t D, int32_t F, float hidden_scale, float* y, uint16_t* hidden_pair, int32_t* pair_written);
/* Q, K and V of the fp32 graph as three gemm32 calls on ONE operand (the second and third with "same operand"):
   out [M, 3 D] = x [M,K] W [3 D,K]^T + bias, the first D columns times qscale.  Classes "gemm32_op_q", "gemm32_op_k", "gemm32_op_v". */
int pf_op_qkv32(pf_engine* e, const float* x, const float* W, const float* bias, int32_t M, int32_t D, int32_t K, float qscale, float* out);
/* Encoder FSMN kernel (f16 V slice of a [B*T, 3D] buffer in, fp32 out): y = dwconv_k(v) + v. */
int pf_op_fsmn_enc(pf_engine* e, const float* v, const float* w, int32_t B, int32_t T, int32_t D, int32_t k, float* y);
/* Decoder FSMN kernel: x += (dwconv_k(tn*m) + tn*m)*m, m = (l < token_num[b]); x in/out [B,L,D]. */
int pf_op_fsmn_dec(pf_engine* e, const float* tn, const float* w, const int32_t* token_num, int32_t B, int32_t L,
                   int32_t D, int32_t k, float* x);
/* The (Bi)LSTM recurrence of the heads on prepared gate inputs, through the functions the heads call:
     xg [B,T3,ndir*4D] = x W_ih^T + b_ih + b_hh (gate order i, f, g, o; directions side by side), whh [ndir,4D,D] fp32,
     hout [B,T3,ndir*D]; D = 512 (and the engine's d_model).
   form 0 = as the f16 timestamp head chooses: the persistent ring when it fits on the device, otherwise the step launches captured
            into a hipGraph that is cached and replayed like the head's;
        1 = plain per-step launches (the hot-word embedder's form);  2 = the f16 ring;  3 = the ring with (hi, lo') pair operands
            (math_mode 3);  4 = one fp32 GEMM + one cell kernel per step (math_mode 1).
   Forms 2 and 3 return PF_ERR_UNSUPPORTED where the ring does not fit (B > 64 at ndir = 2 on 256 compute units); a ring
   time-out is PF_ERR_DEVICE. */
int pf_op_lstm(pf_engine* e, const float* xg, const float* whh, int32_t B, int32_t T3, int32_t D, int32_t ndir, int32_t form,
               float* hout);
/* The tail of the timestamp heads: alphas_raw = relu(sigmoid(hout w + b0) * smooth - noise), alphas = alphas_raw * token_num / sum,
   peak = the running integral with threshold thr (recorded before the reset).  hout [B,T3,W] with W a multiple of 4, w [W],
   b0 [1], token_num [B]; the three outputs [B,T3]. */
int pf_op_us_peak(pf_engine* e, const float* hout, const float* w, const float* b0, float smooth, float noise, const int32_t* token_num,
                  float thr, int32_t B, int32_t T3, int32_t W, float* alphas_raw, float* alphas, float* peak);
/* The pipeline's vocabulary tail: y = log_softmax(x) (two-step form, see k_misc.hip) and the last-index arg-max
   over y — what OfflineRecognizer.cs:139-152 scans.  y_out may be NULL (ids-only variant of the kernel). */
int pf_op_logsoftmax_argmax(pf_engine* e, const float* x, int64_t rows, int32_t V, float* y_out, int64_t* ids_out);
/* LayerNorm over the last dim (eps 1e-12), fp32. */
int pf_op_layernorm(pf_engine* e, const float* x, const float* gamma, const float* beta,
                    int64_t rows, int32_t dim, float* y);
/* softmax(q k^T) v per head, q pre-scaled; q [B,Lq,H*128], k,v [B,Lk,H*128] (fp32 host,
   converted to f16 on device as the pipeline does). */
int pf_op_attention(pf_engine* e, const float* q, const float* k, const float* v,
                    int32_t B, int32_t Lq, int32_t Lk, int32_t heads, float* out);
/* The attention kernels launched the way the pipeline launches them, for conformance tests (tests/attn_ref.py).
   q [B,Lq,H*128], k / v [B,Lk,H*128] ([1,Lk,H*128] with shared_kv) are fp32 host arrays; the op lays them out itself:
     kind    0 = the f16 kernel (k_attn.hip); 1 = the fp32 kernels (MFMA form, or one query per workgroup when the
             output breaks the 16-byte rule); 2 = the fp32 MFMA form writing the (hi | lo') f16 pair, lo' o_ld columns
             behind hi in rows of 2 * o_ld; `out` then receives hi + lo' * 2^-11
     layout  0 = three contiguous matrices; 1 = packed [B*T, 3*Dm] = q | k | v, row stride 3*Dm (Lq == Lk);
             2 = q contiguous, K | V side by side in [B*Lk, ldkv] at column kv_off (ldkv >= kv_off + 2*Dm, both % 8 == 0);
             3 = Q | K in one blocked [rows, 2*Dm] f16 matrix built on the host, V row-major (kind 0, Lq == Lk)
     shared_kv   k / v batch stride 0 (layouts 0 and 2)
     o_ld    output row stride in elements (0 = Dm); form 0 = by shape, 4 / 8 = the 4- / 8-wave workgroup (kind 0)
   Every device operand and its >= 256 rows of slack hold the NaN pattern of its type except the valid elements; the
   output buffer (B*Lq + 256 rows of o_ld elements; 2*o_ld for kind 2) is pre-filled with the 16-bit pattern
   PF_ATTN_CANARY and comes back whole in `raw` (raw_bytes must be its size).  range_out: NULL, or 512 floats = the 256
   {min, max} pairs of the kernel's range output (kind 0; the buffer is NaN-filled before the launch).  *ran = 0 when
   the kind-2 launcher reports that the MFMA form does not apply (nothing was launched), else 1. */
#define PF_ATTN_CANARY 0x4D2B
typedef struct pf_attn_desc { int32_t struct_size, kind, layout, shared_kv, o_ld, form, ldkv, kv_off; } pf_attn_desc;
int pf_op_attention_ex(pf_engine* e, const float* q, const float* k, const float* v, int32_t B, int32_t Lq, int32_t Lk,
                       int32_t heads, const pf_attn_desc* desc, float* out, void* raw, int64_t raw_bytes, float* range_out,
                       int32_t* ran);
/* The encoder's fused Q | K | V projection (d_model 512, 4 heads) and its self-attention as the pipeline launches them
   for long inputs: persistent 256 x 192 GEMM (q scaled by 1/sqrt(128); Q and K in the blocked activation layout, V
   row-major) + the attention kernel reading that layout.  x [B*T, K], w [1536, K] = [Q | K | V] rows, bias [1536] or
   NULL; q/k/v/ctx_out [B*T, 512] (the stored f16 values widened to fp32; each may be NULL). */
int pf_op_qkv_attention(pf_engine* e, const float* x, const float* w, const float* bias, int32_t B, int32_t T, int32_t K,
                        float* q_out, float* k_out, float* v_out, float* ctx_out);
/* DFSMN memory block: y = dwconv_k(v*mask) + v*mask, *mask; v [B,T,D], w [D,k], mask [B,T] or NULL. */
int pf_op_fsmn(pf_engine* e, const float* v, const float* w, const float* mask,
               int32_t B, int32_t T, int32_t D, int32_t k, float* y);
/* CIF integrate-and-fire: H [B,T,D], alphas [B,T+1] -> embeds [B,Lcap,D] (zero padded),
   fire_count [B], token_num [B]; returns L = max fire_count in *L_out.  The counts and *L_out are written before the
   capacity is checked: with Lcap < L the call returns PF_ERR_CAPACITY, leaves embeds untouched and the counts valid
   (Lcap = 0 asks for the counts only; embeds may then be NULL). */
int pf_op_cif(pf_engine* e, const float* H, const float* alphas, int32_t B, int32_t T, int32_t D,
              float threshold, int32_t Lcap, float* embeds, int32_t* fire_count,
              int32_t* token_num, int32_t* L_out);
/* The CIF predictor's alpha stage with the engine's loaded predictor weights, through the function the pipeline runs:
   H [B,T,d_model] (an encoder output) -> conv1d over time (zero padded) + ReLU -> alpha = relu(sigmoid(y . w + b) * smooth - noise);
   alphas [B,T+1], alphas[b,T] = the tail weight.  math_mode 0 rounds H to f16 as the pipeline holds it, math_mode 1 / 3 run the
   fp32 graph; PF_ERR_UNSUPPORTED for math_mode 2 and for SenseVoice models. */
int pf_op_cif_alphas(pf_engine* e, const float* H, int32_t B, int32_t T, float* alphas);
/* Encoder only: speech [B,T,feat] -> H [B,T,512] fp32. */
int pf_op_encoder(pf_engine* e, const float* speech, int32_t B, int32_t T, float* H);

/* ------------------------------------------------------------------------ */
/* 6. Host-side recognizer: same surface as the reference's public classes
 *    OfflineRecognizer (OfflineRecognizer.cs:13-477) and OfflineStream
 *    (OfflineStream.cs:7-121).  Implemented in C++ above the engine.         */
/* ------------------------------------------------------------------------ */
typedef struct pf_recognizer pf_recognizer;
typedef struct pf_stream pf_stream;

/* new OfflineRecognizer(modelFilePath, configFilePath, mvnFilePath, tokensFilePath,
                         modelebFilePath = "", hotwordFilePath = "", batchSize = 1, threadsNum = 1)
   (OfflineRecognizer.cs:23).  modelFilePath names a .pfw container; batchSize/threadsNum are
   accepted and unused exactly as in the reference (quirk Q14); device is the extra argument. */
int pf_recognizer_create(const char* model_path, const char* config_path, const char* mvn_path,
                         const char* tokens_path, const char* modeleb_path,
                         const char* hotword_path, int32_t batch_size, int32_t threads_num,
                         int32_t device, pf_recognizer** out);
void pf_recognizer_dispose(pf_recognizer* r);   /* Dispose(): frees the engine; later calls -> PF_ERR_DISPOSED   */
void pf_recognizer_free(pf_recognizer* r);      /* Dispose() + drops the handle's reference; streams created from it
                                                   stay valid handles (their calls answer PF_ERR_DISPOSED)        */
pf_engine* pf_recognizer_engine(pf_recognizer* r);
/* The recognizer owns a POOL of engines on its device (round 5): GetResults / AddSamples calls of different threads run on
   different engines instead of queueing — the reference's GetResults is unlocked (OfflineRecognizer.cs:110-198).  Engines
   beyond the first are created when a call finds all of them busy, up to $PF_RECOGNIZER_ENGINES (default 2, 1..8); they share
   the device weight image.  Returns how many exist (>= 1), or PF_ERR_DISPOSED.  pf_recognizer_engine hands out engine 0. */
int pf_recognizer_num_engines(pf_recognizer* r);

int pf_recognizer_create_stream(pf_recognizer* r, pf_stream** out);     /* CreateOfflineStream :92 */
/* AddSamples, OfflineStream.cs:36.  `samples` belongs to the caller again when the call returns (the reference's contract): an
   array the recognizer has not seen before has been copied into pinned staging memory by then and its DMA may still be in
   flight — whatever reads the samples later (pf_recognizer_get_results, a second pf_stream_add_samples, pf_stream_free) waits
   for it by itself. */
int pf_stream_add_samples(pf_stream* s, const float* samples, int64_t n);
/* AddSamples for raw PCM (see "PCM intake" above).  The FIRST call on a stream of a recognizer uploads the raw bytes through
   the same copy lane and converts them on the device behind the last DMA piece: the stream then holds exactly what
   pf_stream_add_samples of the converted floats would have left, and the call returns as early.  Every other case (a second
   call, a pf_stream_create stream not adopted yet, PF_RECOGNIZER_DEVICE_STREAMS=0, no device memory) converts on the host
   with the same arithmetic and continues as pf_stream_add_samples.  data == NULL -> PF_ERR_NULL_SAMPLES. */
int pf_stream_add_pcm(pf_stream* s, const void* data, int64_t n_values, const pf_pcm_desc* desc);
/* stream.Hotwords = List<int[]> (flattened ids + per-hotword lengths); n_hotwords < 0 sets null. */
int pf_stream_set_hotwords(pf_stream* s, const int32_t* ids, const int32_t* lens, int32_t n_hotwords);
int pf_stream_get_hotwords(pf_stream* s, int32_t* ids, int32_t ids_cap, int32_t* lens,
                           int32_t lens_cap, int32_t* n_hotwords /* -1 = null */);
int pf_stream_num_feature_floats(pf_stream* s, int32_t* n);  /* OfflineInputEntity.SpeechLength */
void pf_stream_dispose(pf_stream* s);            /* DisposeOfflineStream :441: drops the buffers; the handle stays
                                                    valid and later calls answer PF_ERR_DISPOSED           */
void pf_stream_free(pf_stream* s);               /* releases the handle (and its share of the recognizer).  Idempotent: the
                                                    handle keeps answering PF_ERR_DISPOSED (Dispose + finaliser both
                                                    calling it is safe) until 65 536 younger stream handles have been
                                                    freed, after which its few dozen bytes are handed out again — a
                                                    server creating one stream per utterance does not grow          */

/* GetResults(List<OfflineStream>) (OfflineRecognizer.cs:110): Forward + DecodeMulti.
   Results stay owned by the recognizer until the next GetResults call / dispose. */
int pf_recognizer_get_results(pf_recognizer* r, pf_stream* const* streams, int32_t n_streams);
/* Accessors for result i of the last GetResults: OfflineRecognizerResultEntity
   {Text, TextLen, Tokens, Timestamps} (Model/OfflineRecognizerResultEntity.cs:9-29). */
int pf_result_text(pf_recognizer* r, int32_t i, const char** utf8, int32_t* text_len_utf16);
int pf_result_num_tokens(pf_recognizer* r, int32_t i, int32_t* n);
int pf_result_token(pf_recognizer* r, int32_t i, int32_t j, const char** utf8);
/* timestamp j of result i: n_ints is 2, or 4+ for merged BPE tokens (quirk Q10). */
int pf_result_timestamp(pf_recognizer* r, int32_t i, int32_t j, const int32_t** ints, int32_t* n_ints);
int pf_result_num_timestamps(pf_recognizer* r, int32_t i, int32_t* n);
/* stream.Tokens after Forward (raw ids, OfflineRecognizer.cs:187). */
int pf_stream_tokens(pf_stream* s, const int64_t** ids, int32_t* n);
/* Decoding extras for every engine of the recognizer's pool, present and future (PF_DECODE_*, see pf_engine_set_decode).
   With PF_DECODE_CTC (SenseVoice) GetResults leaves in each stream the COLLAPSED ids as Tokens, one
   [begin, end] pair in milliseconds per token as Timestamps (ms = lfr_n * 10, P = 4 prompt rows:
   begin = ms * max(first - P, 0), end = ms * max(last + 1 - P, 0)) and the token scores; with PF_DECODE_SCORES alone
   Tokens / Timestamps stay as they are and the scores are the [L] per-position row. */
int pf_recognizer_set_decode(pf_recognizer* r, int32_t flags);
/* scores of the stream's last GetResults, parallel to pf_stream_tokens (n = 0 without a decode flag) */
int pf_stream_scores(pf_stream* s, const float** scores, int32_t* n);
/* Alternatives (see "Top-k and n-best").  N = 0: off (K ignored).  N >= 1 (<= PF_NBEST_MAX), K: 1 .. PF_TOPK_MAX (0 = 4):
   PF_DECODE_TOPK with that K on every engine of the pool, present and future, beside the flags of pf_recognizer_set_decode.
   After GetResults each stream carries TokenAlternatives: K (id, log-prob) pairs per entry of Tokens —
     paraformer: per position;  SenseVoice without PF_DECODE_CTC: per frame;
     SenseVoice with PF_DECODE_CTC: those of the FIRST frame of the token's run whose score equals the token's score bit
     for bit (the run's peak frame).
   and, for a paraformer recognizer with N > 1, Alternatives: up to N hypotheses (ids, score, text, tokens) in
   pf_host_nbest order, each decoded by the same DecodeMulti as the result; alternative 0 is the result itself.
   N > 1 on a SenseVoice recognizer -> PF_ERR_UNSUPPORTED (its frames are not independent tokens); any N >= 1 on SeACo too.
   Tokens, Timestamps, Scores and the result text are what they are without it. */
int pf_recognizer_set_nbest(pf_recognizer* r, int32_t N, int32_t K);
/* SenseVoice only (see "CTC beam search"; PF_ERR_UNSUPPORTED otherwise).  N = 0: off.  N >= 1 (<= PF_NBEST_MAX), W = 0
   (max(16, N)) or N .. 64, K = 0 (4) or 1 .. PF_TOPK_MAX: PF_DECODE_CTC_BEAM on every engine of the pool, present and future,
   beside the flags of pf_recognizer_set_decode.  After GetResults each stream's Alternatives holds up to N labelings by
   descending score (ids of their own length, score = the float64 total, text and tokens by the same DecodeMulti as the
   result); TokenAlternatives is filled as with pf_recognizer_set_nbest(1, K).  Tokens, Timestamps, Scores and the result
   text are what they are without it; alternative 0 is the search's best, not necessarily the result. */
int pf_recognizer_set_ctc_beam(pf_recognizer* r, int32_t N, int32_t W, int32_t K);
/* SenseVoice only (see "CTC forced alignment"; PF_ERR_UNSUPPORTED otherwise).  on != 0: PF_DECODE_ALIGN on every engine of
   the pool, present and future, beside the other flags.  A stream's target is set with pf_stream_set_align_ids (token IDS — text
   to ids is the caller's; kept until cleared with n < 0; PF_ERR_INVALID_ARG for an id outside [1, V), PF_ERR_CAPACITY above
   PF_ALIGN_MAX_TOKENS); in a batch a stream without a target is skipped.  After GetResults pf_stream_alignment gives the
   target's [begin, end] pairs in ms (begin = ms * max(first - 4, 0), end = ms * max(last + 1 - 4, 0), ms = lfr_n * 10, as for
   PF_DECODE_CTC), the token scores, the Viterbi score, the log-likelihood and ok; *n = -1 when nothing was aligned for the
   stream, and with ok = 0 the arrays are empty.  With pf_recognizer_set_ctc_beam beside it each Alternative carries the times
   of its own alignment — in its decoded timestamps in place of {0, 0}, and raw ([*n, 2], *n = 0 without) through
   pf_stream_alternative_timestamps — and *loglik, the log of the sum over ALL of its alignments (NaN without).  Tokens,
   Timestamps, Scores, the result text and the alternatives' order and scores are what they are without it.  The pointers stay
   valid until the stream's next GetResults. */
int pf_recognizer_set_align(pf_recognizer* r, int32_t on);
/* SenseVoice only (see "CTC hot words"; PF_ERR_UNSUPPORTED otherwise).  boost > 0: the beam search of
   pf_recognizer_set_ctc_beam is biased towards the batch's hot words by `boost` per matched token; 0 = off; inert until
   pf_recognizer_set_ctc_beam is set.  The hot words of a GetResults call follow the SeACo rule: the union of the batch's
   stream.Hotwords (pf_stream_set_hotwords; a null list fails the call as it does there), and if that is empty the recognizer's
   hot-word file, tokenised as the reference does (per character IndexOf, unknown characters dropped) — a SenseVoice caller who
   needs sentencepiece pieces sets stream.Hotwords ids.  The [1] terminator entry GetHotwords appends is dropped wherever it
   appears.  An engine keeps its automaton while the union is the same.  Alternatives then come in the biased order, each with
   score (biased), hotword_tokens (= matched) and loglik_sum through pf_stream_alternative_hot (0 / NaN when the call ran
   unbiased); Text and Tokens stay what they are.  A hot word that breaks the automaton's limits or holds an id outside
   [1, V) fails GetResults (PF_ERR_RECOGNITION). */
/* Long-audio recognition (see "Voice-activity segmentation"; additions to ABI 6).  cfg != NULL: every GetResults that follows, on
   every engine of the pool, present and future,
     - segments all of the call's streams on the device, where their audio lies (one batched launch set);
     - pools the segments and plans batches of similar length (pf_host_long_plan with batch_max / frame_budget; 0 = 32 / 96000);
     - forwards batch after batch over device pointers into the streams' resident audio, no copy: a segment's ids, text,
       times and scores are exactly what a plain stream holding its sample range gives in that batch position;
     - stitches one result per stream in time order: Text = the segment texts joined by sep_utf8 (NULL = ""), Tokens and the
       raw ids concatenated, every int of every timestamp entry + 10 * b ms (b = the segment's first frame), Scores
       concatenated when a decode flag is set.  A stream with no segment gets empty Text, Tokens and Timestamps and takes
       part in no forward.
   cfg == NULL: off — nothing of this is launched or allocated and every result is bit for bit what it is without it.
   The cut is made in the SAMPLES: a stream must hold its audio on the device (one pf_stream_add_samples / pf_stream_add_pcm
   call); a stream that holds features only (a second AddSamples call, pf_stream_set_speech, PF_RECOGNIZER_DEVICE_STREAMS=0)
   fails the call as PF_ERR_UNSUPPORTED inside Forward's try block ("Offline recognition failed: ...", PF_ERR_RECOGNITION).
   Allowed beside it: PF_DECODE_SCORES, PF_DECODE_CTC, timestamp models, SeACo hot words (the union of the call's
   stream.Hotwords goes to every batch).  PF_ERR_UNSUPPORTED beside it, whichever is set second: pf_recognizer_set_nbest,
   pf_recognizer_set_ctc_beam, pf_recognizer_set_align.  pf_group_* and the streaming classes have no such switch (the streaming
   classes find sentence ends with "Streaming endpointing and the second pass" instead, and may hand each sentence to a recognizer
   WITHOUT this switch).
   PF_ERR_INVALID_ARG as for pf_vad_config; PF_ERR_UNSUPPORTED for a snip_edges = true front-end. */
int pf_recognizer_set_vad(pf_recognizer* r, const pf_vad_config* cfg, int32_t batch_max, int64_t frame_budget, const char* sep_utf8);
/* The FSMN-VAD model score for long-audio recognition (see "Voice-activity segmentation, model score"): pfw_path = a `.pfw` of
   kind "fsmnvad", loaded once and attached to every engine of the pool, present and future; NULL clears.  Inert until
   pf_recognizer_set_vad, and may be set before or after it.  The thresholds of pf_vad_model_config are the caller's to pass to
   pf_recognizer_set_vad.  Errors as pf_vad_model_load and pf_engine_set_vad_model. */
int pf_recognizer_set_vad_model(pf_recognizer* r, const char* pfw_path);
/* Punctuation of every GetResults that follows (see "Punctuation"): pfw_path = a `.pfw` of kind "cttransformer", loaded once
   and attached to every engine of the pool; NULL clears.  GetResults then punctuates each stream's final text (with
   pf_recognizer_set_vad: the stitched text), all streams of the call in one pf_engine_punctuate, and keeps the result on the
   stream; Text, Tokens and Timestamps of the result are what they are without it.  Alternatives are not punctuated; pf_group_*
   has no such switch; the streaming classes have pf_online_recognizer_set_punc_model (a causal model).  Errors as pf_punc_model_load.
   pf_stream_punctuated: the punctuated text, the mark of every word (punc_list index) and the word count of the stream's last
   GetResults ("" / 0 without a model); each output optional; valid until the stream's next GetResults.
   pf_stream_sentence: sentence i: its words [word_begin, word_end), its punctuated text and, when the result has exactly one
   Timestamps entry per word and they are not all the {0, 0} placeholders of a model without timestamps (*has_time), [begin of
   its first word, end of its last] in ms. */
int pf_recognizer_set_punc_model(pf_recognizer* r, const char* pfw_path);
/* Speaker labels of every long-audio GetResults that follows (see "Speaker labels"): pfw_path = a `.pfw` of kind "campplus",
   loaded once and attached to every engine of the pool, present and future; NULL clears.  cfg == NULL: the defaults.  Inert
   until pf_recognizer_set_vad, and may come before or after it.  GetResults then, behind the segmentation and on the fbank rows
   it staged (no second fbank), plans the windows of all of the call's streams, embeds them (as many windows per forward as keep the activations within 2 GiB: about
   1000 windows of 150 frames at the released dimensions), computes one cosine block per stream on the device and clusters each stream on the host.  Text,
   Tokens, Timestamps, Scores, Segments, Punctuated and Sentences are what they are without it.  pf_group_* and the streaming
   classes have no such switch.  Errors as pf_spk_model_load; PF_ERR_INVALID_ARG for a cfg outside its ranges or a model whose
   n_mels is not the front-end's.
   Of the stream's last long-audio GetResults, valid until its next one (0 / nothing without a model):
   pf_stream_num_speakers; pf_stream_segment_speaker: the label of segment i (as pf_stream_segment counts them; -1: the stream
   has no window at all); pf_stream_speaker_centroid: out [cap >= E] = speaker spk's centroid, the L2-normalised mean of its
   windows' L2-normalised embeddings, for matching against enrolled voices (*E optional; out NULL with cap 0 to learn it);
   pf_stream_spk_window: window i in ms and its label. */
int pf_recognizer_set_spk_model(pf_recognizer* r, const char* pfw_path, const pf_spk_config* cfg);
int pf_stream_num_speakers(pf_stream* s, int32_t* n);
int pf_stream_segment_speaker(pf_stream* s, int32_t i, int32_t* spk);
int pf_stream_speaker_centroid(pf_stream* s, int32_t spk, float* out, int32_t cap, int32_t* E);
int pf_stream_num_spk_windows(pf_stream* s, int32_t* n);
int pf_stream_spk_window(pf_stream* s, int32_t i, int32_t* begin_ms, int32_t* end_ms, int32_t* label);
int pf_stream_punctuated(pf_stream* s, const char** text_utf8, const int32_t** punc_ids, int32_t* n_words);
int pf_stream_num_sentences(pf_stream* s, int32_t* n);
int pf_stream_sentence(pf_stream* s, int32_t i, int32_t* word_begin, int32_t* word_end, int32_t* has_time, int32_t* begin_ms,
                       int32_t* end_ms, const char** text_utf8);
/* The segments of the stream's last GetResults in time order (0 without pf_recognizer_set_vad): [begin_ms, end_ms) on the
   stream's clock, where it ran (batch, row of the plan), its share [tok_begin, tok_end) of pf_stream_tokens / pf_stream_scores
   / pf_stream_timestamp, and its own text; each output optional.  Valid until the stream's next GetResults. */
int pf_stream_num_segments(pf_stream* s, int32_t* n);
int pf_stream_segment(pf_stream* s, int32_t i, int32_t* begin_ms, int32_t* end_ms, int32_t* batch, int32_t* row, int32_t* tok_begin,
                      int32_t* tok_end, const char** text_utf8);
int pf_recognizer_set_hotword_boost(pf_recognizer* r, float boost);
int pf_stream_alternative_hot(pf_stream* s, int32_t i, int32_t* hotword_tokens, double* loglik_sum);
/* SenseVoice only (see "CTC language model"; PF_ERR_UNSUPPORTED otherwise).  An ARPA n-gram LM fused into the beam search of
   pf_recognizer_set_ctc_beam with weight alpha, per-token bonus beta and flags (PF_LM_EOS); inert until
   pf_recognizer_set_ctc_beam is set; arpa_path NULL or "" clears it.  The file is read once, against the recognizer's token
   table (pf_host_lm_from_arpa with oov = -10); each engine of the pool uploads the image on first use.  Alternatives then come
   in the fused order, each with its score (fused), lm_sum and loglik_sum through pf_stream_alternative_lm (NaN when the call
   ran without a model); beside pf_recognizer_set_hotword_boost both terms enter one search.  Text and Tokens of the result
   stay the greedy ones.  Errors as pf_host_lm_from_arpa and pf_engine_set_ctc_lm (the installed model stays). */
int pf_recognizer_set_lm(pf_recognizer* r, const char* arpa_path, float alpha, float beta, int32_t flags);
int pf_stream_alternative_lm(pf_stream* s, int32_t i, double* lm_sum, double* loglik_sum);
/* Paraformer only (see "N-best search"; PF_ERR_UNSUPPORTED for a SenseVoice or SeACo model; "off" — W = 0, boost = 0, a NULL or
   empty path — is always accepted).  pf_recognizer_set_nbest_search: W = 0 off, else 1 .. PF_NBEST_MAX: with
   pf_recognizer_set_nbest(N > 1, K) in force (inert until then) every engine of the pool, present and future, runs the beam
   search of width max(W, N) on the device and Alternatives come from its result block in the FUSED order — the host
   enumeration (pf_host_nbest) is skipped — each decoded by the same DecodeMulti, with its score, and hotword_tokens /
   loglik_sum / lm_sum through pf_stream_alternative_hot / pf_stream_alternative_lm: score == (loglik_sum + boost *
   hotword_tokens) + lm_sum bit for bit (lm_sum 0 without a model).  Text, Tokens, Timestamps, Scores and TokenAlternatives are
   untouched.  PF_ERR_UNSUPPORTED beside pf_recognizer_set_vad, whichever is set second.
   pf_recognizer_set_nbest_lm: an ARPA file read once against the recognizer's token table (as pf_recognizer_set_lm; each engine
   uploads it on first use), alpha, beta, flags as pf_engine_set_nbest_lm.  pf_recognizer_set_nbest_hotword_boost: boost per
   matched token of a hot word (finite, >= 0); the hot words of a GetResults call come from where pf_recognizer_set_hotword_boost
   reads them: the union of its streams' Hotwords, else the hot-word file's.  pf_recognizer_set_lm,
   pf_recognizer_set_hotword_boost and pf_recognizer_set_ctc_beam keep refusing a paraformer. */
int pf_recognizer_set_nbest_search(pf_recognizer* r, int32_t W);
int pf_recognizer_set_nbest_lm(pf_recognizer* r, const char* arpa_path, float alpha, float beta, int32_t flags);
int pf_recognizer_set_nbest_hotword_boost(pf_recognizer* r, float boost);
int pf_stream_set_align_ids(pf_stream* s, const int64_t* ids, int32_t n);
int pf_stream_alignment(pf_stream* s, const int32_t** begin_end, const float** tok_score, int32_t* n, float* path_score,
                        double* loglik, int32_t* ok);
int pf_stream_alternative_timestamps(pf_stream* s, int32_t i, const int32_t** begin_end, int32_t* n, double* loglik);
/* ids / val: [*n_tokens, *K], parallel to pf_stream_tokens; slots past a position's n hold -1 / -inf.  *n_tokens = 0
   without pf_recognizer_set_nbest.  The pointers stay valid until the stream's next GetResults. */
int pf_stream_token_alternatives(pf_stream* s, const int64_t** ids, const float** val, int32_t* n_tokens, int32_t* K);
int pf_stream_num_alternatives(pf_stream* s, int32_t* n);
/* alternative i: its ids [*n_ids], score, text and the number of decoded tokens (each optional) */
int pf_stream_alternative(pf_stream* s, int32_t i, const int64_t** ids, int32_t* n_ids, double* score, const char** text_utf8,
                          int32_t* n_tokens);
int pf_stream_alternative_token(pf_stream* s, int32_t i, int32_t j, const char** utf8);

/* ABI 6: the rest of OfflineStream's public surface (OfflineStream.cs:20-34).  Only the reference's own Forward touches
   these members, but "same public signatures" means a caller may.
   new OfflineStream(mvnFilePath, confEntity) (:20-28): a stream that belongs to no recognizer yet; the arguments are
   confEntity.frontend_conf's fields (0 / NULL = the FrontendConfEntity default).  Its AddSamples calls are kept on the host
   and replayed by the first GetResults that receives it; a front-end other than that recognizer's -> PF_ERR_UNSUPPORTED
   (raised by that GetResults inside Forward's try block: "Offline recognition failed"). */
int pf_stream_create(const char* mvn_path, int32_t fs, int32_t n_mels, int32_t lfr_m, int32_t lfr_n, int32_t snip_edges,
                     float dither, const char* window, pf_stream** out);
int pf_stream_set_tokens(pf_stream* s, const int64_t* ids, int32_t n);          /* Tokens { set; }      :32 */
int pf_stream_num_timestamps(pf_stream* s, int32_t* n);                          /* Timestamps { get; }  :33 */
int pf_stream_timestamp(pf_stream* s, int32_t j, const int32_t** ints, int32_t* n_ints);
int pf_stream_set_timestamps(pf_stream* s, const int32_t* ints, const int32_t* lens, int32_t n);   /* Timestamps { set; } */
/* OfflineInputEntity { Speech, SpeechLength } (:30; Model/OfflineInputEntity.cs).  get: *n_floats = -1 when Speech is null,
   else the float count (PF_ERR_CAPACITY with the count reported when cap is smaller); a stream whose samples live on the
   device is brought to the host form (features computed and read back).  set: n_floats < 0 sets Speech = null;
   speech_length is stored as given (the reference's two setters are independent). */
int pf_stream_get_speech(pf_stream* s, float* out, int64_t cap, int32_t* n_floats);
int pf_stream_set_speech(pf_stream* s, const float* speech, int32_t n_floats, int32_t speech_length);

/* ------------------------------------------------------------------------ */
/* 7. Streaming path: the reference's OnlineRecognizer / OnlineStream
 *    (AliParaformerAsr/OnlineRecognizer.cs:14-542, OnlineStream.cs:7-358).  The chunking, the feature caches,
 *    DynamicMask and the carried-integrator CIF are host code as in the reference (C++ here); the two ONNX
 *    sessions (OnlineModel.cs:23-31) are the device seams pf_online_encoder / pf_online_decoder.          */
/* ------------------------------------------------------------------------ */
typedef struct pf_online_recognizer pf_online_recognizer;
typedef struct pf_online_stream pf_online_stream;
/* new OnlineRecognizer(encoderFilePath, decoderFilePath, configFilePath, mvnFilePath, tokensFilePath, threadsNum)
   (OnlineRecognizer.cs:22): encoder_path names ONE .pfw container holding both graphs' tensors; decoder_path is
   accepted and unused; device is the extra argument. */
int pf_online_recognizer_create(const char* encoder_path, const char* decoder_path, const char* config_path,
                                const char* mvn_path, const char* tokens_path, int32_t threads_num, int32_t device,
                                pf_online_recognizer** out);
void pf_online_recognizer_dispose(pf_online_recognizer* r);
void pf_online_recognizer_free(pf_online_recognizer* r);
pf_engine* pf_online_recognizer_engine(pf_online_recognizer* r);
int pf_online_create_stream(pf_online_recognizer* r, pf_online_stream** out);          /* CreateOnlineStream :27 */
int pf_online_stream_add_samples(pf_online_stream* s, const float* samples, int64_t n); /* OnlineStream.AddSamples */
/* GetResults(List<OnlineStream>) (:41-48): one chunk per stream that has 60 fbank frames ready; texts are kept for
   the calling thread until its next call. */
int pf_online_get_results(pf_online_recognizer* r, pf_online_stream* const* streams, int32_t n_streams);
int pf_online_result_text(pf_online_recognizer* r, int32_t i, const char** utf8);
int pf_online_stream_tokens(pf_online_stream* s, const int64_t** ids, int32_t* n);
void pf_online_stream_dispose(pf_online_stream* s);
void pf_online_stream_free(pf_online_stream* s);
/* ---- Streaming endpointing and the second pass (additions to ABI 6; opt-in: without pf_online_recognizer_set_endpoint nothing
   of this is launched or allocated and every streaming result is bit for bit what it is without it) ----
   The detector of "Voice-activity endpointing, streaming" runs inside pf_online_get_results over the fbank rows of the CALLER's
   audio (9600 samples at a time, as AddSamples hands them on; not the chunk of silence the constructor queues, not the repeated
   first frame): one launch set for all the call's streams that have new frames — rows gathered, one upload, the level launch,
   the endpoint launch, one read-back.  The state blocks live in one device buffer of the recognizer.
   An event closes a sentence, at chunk granularity: its first-pass text is the online model's text after the ids of this
   call's chunk were appended; the stream's decoder context is then reset (Tokens cleared, FSMN caches zeroed, the CIF carry
   and the feature cache back to their initial values, the position index 0) while the fbank rows and the LFR splice cache
   stay: the audio is continuous.  At a forced cut a token may straddle the cut.  pf_online_result_text keeps returning the text
   of the OPEN sentence: the tokens since the last reset.
   Second pass: the sentences that closed in one call, pooled over its streams in the call's stream order and then in time order,
   each become one plain offline stream holding the caller's samples [160 b, min(n_samples, 160 e)) and go through ONE GetResults
   of the attached offline recognizer (the batch is part of the definition: quirk Q2).  text is that result; without a second
   pass text equals first_pass.  What the offline recognizer has set (punctuation, n-best, timestamps) simply applies;
   PF_ERR_UNSUPPORTED for one with pf_recognizer_set_vad on.  The offline recognizer must outlive its use here.
   pf_online_stream_input_finished: the cached samples go through the front-end, the last ones zero-padded to one chunk, so the
   online model decodes the tail too; the pf_online_get_results that has decoded the last chunk flushes the detector (frames:
   ceil(n_samples / 160)).  A later pf_online_stream_add_samples: PF_ERR_INVALID_ARG.
   Times are milliseconds in the caller's audio.  pf_online_stream_sentence_result: the offline stream that produced sentence j
   (borrowed: valid until the online stream is freed; NULL without a second pass) — every pf_stream_* getter works on it, times
   inside it are relative to begin_ms. */
int pf_online_recognizer_set_endpoint(pf_online_recognizer* r, const pf_endpoint_config* cfg);   /* NULL = off */
/* The FSMN-VAD model score as the detector's level ("Voice-activity endpointing, streaming, model score"): loads the `.pfw` of
   kind "fsmnvad" as pf_recognizer_set_vad_model does and attaches it to the recognizer's engine; NULL detaches.  The stream
   launch (profile class "vadnet_stream") then runs where the level launch runs and hands its released counts to the endpoint
   launch: still one upload and one read-back per call, and a flush releases the held-back levels and flushes the detector in
   the same launch set, also when the call brought no new rows.  The network states live in a second device buffer of the
   recognizer, indexed by the detector's slot.  Inert until pf_online_recognizer_set_endpoint; pass pf_endpoint_model_config's
   thresholds there.  Errors as pf_vad_model_load and pf_engine_set_vad_model (input width, snip_edges); PF_ERR_UNSUPPORTED for a
   model beyond the LDS limit, and for attaching or detaching while a live stream has already fed the detector: two kinds of
   level must not meet in one state block. */
int pf_online_recognizer_set_endpoint_model(pf_online_recognizer* r, const char* pfw_path);     /* NULL = the energy level */
int pf_online_recognizer_set_second_pass(pf_online_recognizer* r, pf_recognizer* offline);      /* NULL = none */
int pf_online_stream_input_finished(pf_online_stream* s);
int pf_online_stream_num_sentences(pf_online_stream* s, int32_t* n);
int pf_online_stream_sentence(pf_online_stream* s, int32_t j, int32_t* begin_ms, int32_t* end_ms, int32_t* kind,
                              const char** first_pass_utf8, const char** text_utf8);
int pf_online_stream_sentence_result(pf_online_stream* s, int32_t j, pf_stream** offline_stream);
int pf_online_stream_in_speech(pf_online_stream* s, int32_t* in_speech, int32_t* begin_ms);
/* ---- Streaming token times and scores (additions to ABI 6; opt-in: without pf_online_recognizer_set_token_info(r, 1) every
   streaming call makes the launches and returns the bytes it does without it) ----
   With the mode on a chunk step stays on the device from the encoder to the ids (Engine::online_step): the carried CIF runs
   as a kernel on a per-stream state block (k_cif_stream.hip; the host statement is pf_host_online_cif_step), the FSMN caches
   live in the stream's slot of a device buffer, and only the fire counts and fire entries cross to the host in between.  The
   ids are the ids of the mode-off path.  token_info[i] describes Tokens[i], index for index (n == number of Tokens):
     id       Tokens[i]
     flags    PF_ONLINE_TOKEN_FIRED: a token this stream's integrator fired.  0 for the constructor's two leading zeros and for
              the positions a stream receives because ALL ids of a decoder batch are appended to every stream of the call
              (OnlineRecognizer.cs:389); those positions still carry their arg-max score.
     entry    the walked entry of [carry ; chunk] that completed the token: 0 the carry, j the chunk position j - 1; -1 unfired
     score    the log-probability of id, bit for bit what pf_online_decoder stores at [b, l, id] of its log-probs
     time_ms  with PF_ONLINE_TOKEN_TIMED, else -1.  THE START OF THE 60 ms FRAME IN WHICH THE INTEGRATOR CROSSED THE THRESHOLD,
              in the caller's audio.  It is NOT a word boundary and has not been validated on real speech (there is no corpus
              here).  It comes from provenance: every fbank row carries the caller-sample index of its frame start (row r of a
              chunk whose first caller sample is c: c + 160 r; rows of the constructor's chunk of silence: none); the repeated
              first row, the LFR splice row and the ten cached feature rows carry what they copy (after a sentence reset the
              cached ten carry none); an LFR frame takes the index of its first row.  A token fired at chunk position p takes
              the first position >= p of that chunk whose frame has an index (none: the caller samples that have gone through
              the front-end so far); a token fired on the carry takes the time of position hi - 1 = 14 of the previous chunk.
              time_ms = floor(index * 1000 / fs).  The rows pf_online_stream_input_finished pads behind the caller's
              last sample keep the frame grid of their chunk, so a token fired there can report a time up to 600 ms past
              the end of the caller's audio.
   A sentence closed by the endpoint detector keeps the token info of its first pass (Tokens is cleared at the reset):
   pf_online_stream_sentence_tokens.  The pointers stay valid until the stream's next pf_online_get_results or its free.
   pf_online_recognizer_set_token_info: PF_ERR_UNSUPPORTED once a live stream of the recognizer has decoded a chunk (host-carried
   and device-carried state must not meet in one stream); on == 0 on a fresh recognizer is a no-op.  With the mode off
   pf_online_stream_token_info returns n == 0.  The streams' decoder state is then not readable from the host.
   With the mode on a stream may be passed ONCE per pf_online_get_results (a stream's slot is written by one workgroup set per
   launch): a list that names a stream twice is refused with PF_ERR_INVALID_ARG before any stream's chunk is taken.  The
   mode-off path accepts such a list, as the reference does. */
typedef struct { int64_t id; int32_t time_ms; int32_t entry; float score; int32_t flags; } pf_online_token;
#define PF_ONLINE_TOKEN_FIRED 1   /* this position is a token this stream fired (not the two leading zeros, not batch padding) */
#define PF_ONLINE_TOKEN_TIMED 2   /* time_ms is set */
int pf_online_recognizer_set_token_info(pf_online_recognizer* r, int32_t on);
int pf_online_stream_token_info(pf_online_stream* s, const pf_online_token** toks, int32_t* n);   /* n == number of Tokens, index for index */
int pf_online_stream_sentence_tokens(pf_online_stream* s, int32_t j, const pf_online_token** toks, int32_t* n);
/* ---- Streaming punctuation on the recogniser (additions to ABI 6; see "Punctuation, streaming"; opt-in: without
   pf_online_recognizer_set_punc_model nothing of it is launched, allocated or changed) ----
   pf_online_recognizer_set_punc_model: pfw_path = a causal `.pfw` of kind "cttransformer", loaded once and attached to the
   recogniser's engine; NULL or "" detaches and frees.  max_context 2 .. PF_PUNC_STREAM_MAX_CONTEXT, 0 = the default.  Every
   pf_online_get_results then, behind the chunk step and the endpoint pass, gathers the newly COMMITTED words of its streams
   (pf_host_online_committed_words) and marks them in ONE launch (profile class "punc_stream"); a stream's keys and values stay
   in its slot of a device buffer; a call with no new word and no flush launches nothing.  Text, Tokens, TokenInfo and the
   sentences' text are what they are without it.  When the endpoint detector closes a sentence its remaining words, a held-back
   one included, go in with the flush before the decoder context is reset, and the next sentence starts a fresh context; the
   pf_online_get_results that has decoded the last chunk after pf_online_stream_input_finished flushes likewise.  The flush's
   edit is applied to the newest word's mark.  PF_ERR_UNSUPPORTED: a model that is not causal; a live stream holds punctuation
   state.  PF_ERR_RECOGNITION: the committed words of a call do not begin with the last call's.
   pf_online_stream_punctuated: of the last pf_online_get_results, the open text under the marks of its committed words (a
   held-back word appended raw), the mark and the flags (bit 0 sentence end, bit 1 forced restart) of every committed word.
   pf_online_stream_sentence_punctuated: the same for finished sentence j.  Each output optional; valid until the stream's next
   pf_online_get_results or its free; "" / 0 without a model. */
int pf_online_recognizer_set_punc_model(pf_online_recognizer* r, const char* pfw_path, int32_t max_context);
int pf_online_stream_punctuated(pf_online_stream* s, const char** text_utf8, const int32_t** punc_ids, const int32_t** punc_flags,
                                int32_t* n_words);
int pf_online_stream_sentence_punctuated(pf_online_stream* s, int32_t j, const char** text_utf8, const int32_t** punc_ids, int32_t* n_words);
/* Device seams = the two InferenceSession.Run calls (OnlineRecognizer.cs:83, :296).
   encoder: speech [B,Tc,560] (scaled + position-encoded by the caller) -> enc [B,Tc,512], alphas [B,Tc].
   decoder: enc, acoustic_embeds [B,L,512] + lengths, in_cache [n_caches][B,512,10] -> log-probs [B,L,V] (optional),
            last-index arg-max ids [B,L], out_cache [n_caches][B,512,10]. */
int pf_online_encoder(pf_engine* e, const float* speech, int32_t B, int32_t Tc, float* enc_out, float* alphas_out);
int pf_online_decoder(pf_engine* e, const float* enc, int32_t B, int32_t Tc, const float* embeds, int32_t L,
                      const int32_t* embeds_len, const float* caches_in, int32_t n_caches, float* logits_out,
                      int64_t* ids_out, float* caches_out);
/* Host pieces exposed for parity tests (pure CPU): OnlineWavFrontend.ApplyLfr (:63-80), SinusoidalPositionEncoder
   (:152-188, in place), the per-stream CIF of PredictorProj (OnlineRecognizer.cs:152-197), DynamicMask
   (OnlineModel.cs:141-165, in place), DecodeMulti (:405-437). */
int pf_host_online_lfr(const float* fbank, int32_t t80, int32_t lfr_m, int32_t lfr_n, float* out, int64_t cap, int32_t* t_lfr);
int pf_host_online_posenc(float* x, int32_t timesteps, int32_t dim, int32_t start_idx);
int pf_host_online_dynamic_mask(float* alphas, int32_t n);
int pf_host_online_cif(const float* hiddens, const float* alphas, int32_t n, int32_t D, float threshold, float* fired,
                       int32_t fired_cap, int32_t* n_fired, float* carry_alpha, float* carry_hidden);
/* The carried CIF of one chunk step (k_cif_stream.hip), host statement and device op, bit-equal in every output and state byte.
   state: one stream's block of pf_host_online_cif_state_bytes(D) bytes = hidden [D] fp32 (the carried frame, already divided by
   the carried integrate) | the carried integrate, one equal copy per 256 channels, padded to four cells; zero-filled = the
   constructor's state.  The step walks [carry ; Tc frames]: chunk positions < lo and >= hi with alpha 0 (DynamicMask: lo 5, hi
   15), fire on !(alpha + integrate < threshold), products and sums rounded separately, the new carry = frames / integrate when
   integrate > 0, else frames.  reset != 0: the walk starts from a zero block.  fired [cap, D] (rows at and beyond count zero),
   fire_entry [cap] (0 = the carry, j = chunk position j - 1; -1 at and beyond count).  The op takes B streams (states [B,
   state_bytes], enc [B, Tc, D], alphas [B, Tc], reset [B]) in ONE launch through the staging kit with its guards on every output.
   PF_ERR_INVALID_ARG: null pointers, cap < Tc + 1, D % 4 != 0, B <= 0, Tc <= 0. */
int pf_host_online_cif_state_bytes(int32_t D, int64_t* bytes);
int pf_host_online_cif_step(void* state, const float* hiddens, const float* alphas, int32_t Tc, int32_t D, float threshold, int32_t lo,
                            int32_t hi, int32_t reset, float* fired, int32_t* fire_entry, int32_t cap, int32_t* count);
int pf_op_online_cif_step(pf_engine* e, void* states, const float* enc, const float* alphas, const int32_t* reset, int32_t B, int32_t Tc,
                          int32_t D, float threshold, int32_t lo, int32_t hi, float* fired, int32_t* fire_entry, int32_t cap,
                          int32_t* counts);
int pf_host_online_decode(const char* const* tokens, int32_t n_tokens, const int64_t* ids, int32_t n_ids, char* out,
                          int32_t cap);

/* Host text stage exposed for parity tests (pure CPU, no device): */
/* time_stamp_lfr6_onnx (OfflineRecognizer.cs:200-302): returns count of [begin,end] ms pairs
   written to out_pairs (cap pairs), or a negative status (no fire -> PF_ERR_RECOGNITION). */
int pf_host_timestamps(const float* us_cif_peak, int32_t n, const int64_t* tokens, int32_t n_tokens,
                       int32_t* out_pairs, int32_t cap_pairs);
/* GetHotwords (OfflineRecognizer.cs:72-90) over in-memory token table / hotword lines. */
int pf_host_hotword_ids(const char* const* tokens, int32_t n_tokens, const char* const* lines,
                        int32_t n_lines, int32_t* ids, int32_t ids_cap, int32_t* lens,
                        int32_t lens_cap, int32_t* n_hotwords);
/* DecodeMulti for one stream (OfflineRecognizer.cs:304-418) over an in-memory token table.
   timestamps: flattened ints + per-entry lengths. Result is read with pf_result_* on the
   returned scratch recognizer-less decoder object. */
typedef struct pf_decoded pf_decoded;
int pf_host_decode(const char* const* tokens, int32_t n_tokens, const int64_t* ids, int32_t n_ids,
                   const int32_t* ts_ints, const int32_t* ts_lens, int32_t n_ts, pf_decoded** out);
int pf_decoded_text(pf_decoded* d, const char** utf8, int32_t* text_len_utf16);
int pf_decoded_num_tokens(pf_decoded* d, int32_t* n);
int pf_decoded_token(pf_decoded* d, int32_t j, const char** utf8);
int pf_decoded_num_timestamps(pf_decoded* d, int32_t* n);
int pf_decoded_timestamp(pf_decoded* d, int32_t j, const int32_t** ints, int32_t* n_ints);
void pf_decoded_free(pf_decoded* d);

/* ---- Examples harness helpers (AliParaformerAsr.Examples/Utils/AudioHelper.cs) ---------------------------
   pf_host_wav_read  = GetFileSample (:12-32) for RIFF/WAVE files: decode to float (NAudio AudioFileReader
   conversions), resample + down-mix to 16 kHz mono ONLY when the file's rate is not 16 kHz (upstream quirk: a
   16 kHz stereo file is returned interleaved); a missing file yields one zero sample.  Call with out == NULL to
   learn *n_out.  pf_host_resample = Resample(source, srIn, srOut, channels) (:223-279).
   pf_host_is_audio = IsAudioByHeader (:286-340) restricted to RIFF/WAVE. */
int pf_host_wav_read(const char* path, float* out, int64_t cap, int64_t* n_out, int32_t* sample_rate,
                     int32_t* channels, double* duration_ms);
int pf_host_resample(const float* src, int64_t n, int32_t sr_in, int32_t sr_out, int32_t channels, float* out,
                     int64_t cap, int64_t* n_out);
int pf_host_is_audio(const char* path, int32_t* is_audio);
/* The header walk of pf_host_wav_read WITHOUT the sample loop: what the file holds (desc: format, rate, channels; flags 0) and
   where (data_offset / data_bytes of the payload inside the file, data_bytes clamped to the file; n_values = data_bytes /
   bytes per value), so a caller hands the payload over raw (pf_stream_add_pcm, pf_recognize_pcm).  Each output may be NULL.
   PF_ERR_IO missing file, PF_ERR_FORMAT not RIFF/WAVE or no fmt / data chunk, PF_ERR_UNSUPPORTED other sample formats. */
int pf_host_wav_info(const char* path, pf_pcm_desc* desc, int64_t* data_offset, int64_t* data_bytes, double* duration_ms);

#ifdef __cplusplus
}
#endif
#endif /* PARAFORMER_HIP_H_ */
