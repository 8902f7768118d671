// ParaformerHip.cs — P/Invoke declarations of libparaformer_hip.so (include/paraformer_hip.h, PF_ABI_VERSION 6).
// Drop into the reference project (AliParaformerAsr/Native/) — see csharp/README.md.  Not compiled in the build
// image of this repository (no .NET toolchain); the same entry points are exercised through the Python ctypes
// binding aliparaformerasr_amd/_native.py by tests/.
using System;
using System.Runtime.InteropServices;

namespace AliParaformerAsr.Native
{
    /// <summary>pf_engine_config (paraformer_hip.h): replaces OfflineModel.initModel's SessionOptions
    /// (OfflineModel.cs:35-70) and FrontendConfEntity (Model/FrontendConfEntity.cs:7-15).</summary>
    [StructLayout(LayoutKind.Sequential)]
    internal struct PfEngineConfig
    {
        public int struct_size, device;
        public IntPtr weights_path, weights_host, weights_device;
        public long weights_bytes;
        public IntPtr mvn_path, cmvn_shift, cmvn_scale;
        public int cmvn_dim;
        public int fs, n_mels, lfr_m, lfr_n, snip_edges;
        public float dither;
        public IntPtr window;
        public int use_itn;
        public int frame_length_ms, frame_shift_ms, dither_seed;
        /// <summary>0 = f16 MFMA (model.onnx semantics, default), 1 = fp32 MFMA parity mode, 2 = dynamic int8 as the
        /// reference's default model.int8.onnx computes (Examples/Program.cs:98-101): Linear layers on the int8 MFMA,
        /// 3 = "exact" at matrix-core speed (ABI 5): the fp32 graph with every large Linear as three f16 MFMA products of
        /// (hi, lo) operand pairs — token-identical to fp32 on the benchmark batches.</summary>
        public int math_mode;
        public int reserved0, reserved1, reserved2;
    }

    /// <summary>pf_pcm_desc: what a block of raw interleaved PCM holds (paraformer_hip.h "PCM intake").  format: 1 u8, 2 s16,
    /// 3 s24, 4 s32, 5 float32, 6 float64, 7 A-law, 8 mu-law; flags: PF_PCM_DOWNMIX_ALWAYS = 1.</summary>
    [StructLayout(LayoutKind.Sequential)]
    internal struct PfPcmDesc
    {
        public int struct_size, format, sample_rate, channels, flags, reserved0, reserved1, reserved2;
        internal static PfPcmDesc Of(int format, int sampleRate, int channels, bool downmixAlways = false) => new PfPcmDesc
        {
            struct_size = Marshal.SizeOf<PfPcmDesc>(), format = format, sample_rate = sampleRate, channels = channels,
            flags = downmixAlways ? ParaformerHip.PF_PCM_DOWNMIX_ALWAYS : 0,
        };
    }

    /// <summary>pf_vad_config: the voice-activity detector's configuration (paraformer_hip.h "Voice-activity segmentation");
    /// pf_vad_default fills in the stated defaults, which nobody has validated on real speech.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PfVadConfig
    {
        public int struct_size, floor_pct, margin_q, abs_level, window, on_count, off_count, pad_begin, pad_end, min_speech, max_len,
                   split_search, reserved0, reserved1, reserved2, reserved3;
    }

    /// <summary>pf_endpoint_config: the streaming endpoint detector's configuration (paraformer_hip.h "Voice-activity endpointing,
    /// streaming"); pf_endpoint_default fills in the stated defaults, which nobody has validated on real speech.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PfEndpointConfig
    {
        public int struct_size, rise, margin_q, abs_level, window, on_count, off_count, pad_begin, pad_end, end_silence, min_speech,
                   max_len, reserved0, reserved1, reserved2, reserved3;
    }

    /// <summary>pf_spk_config: the speaker labels' configuration (paraformer_hip.h "Speaker labels"); pf_spk_default fills in the
    /// stated defaults, which nobody has validated on real speech.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PfSpkConfig
    {
        public int struct_size, win, shift, min_frames;
        public float threshold;
        public int num_speakers, min_cluster, reserved0, reserved1, reserved2, reserved3, reserved4;
    }

    /// <summary>pf_batch_out: capacities in, L / V / cif_peak_len and the filled buffers out.</summary>
    [StructLayout(LayoutKind.Sequential)]
    internal struct PfBatchOut
    {
        public int struct_size, l_cap;
        public long logits_cap, cif_peak_cap;
        public IntPtr token_ids, token_num, logits, cif_peak;
        public int L, V, cif_peak_len, reserved;
    }

    internal static class ParaformerHip
    {
        private const string Lib = "paraformer_hip";   // libparaformer_hip.so next to the assembly / on LD_LIBRARY_PATH

        internal const int PF_OK = 0, PF_ERR_INVALID_ARG = -1, PF_ERR_DEVICE = -2, PF_ERR_IO = -3, PF_ERR_FORMAT = -4,
                           PF_ERR_CAPACITY = -5, PF_ERR_UNSUPPORTED = -6, PF_ERR_DISPOSED = -7, PF_ERR_TOKENS = -8,
                           PF_ERR_NULL_SAMPLES = -9, PF_ERR_RECOGNITION = -10;

        [DllImport(Lib)] internal static extern int pf_version();
        [DllImport(Lib)] internal static extern IntPtr pf_last_error();

        // ---- engine (replaces InferenceSession + OnlineFbank) -------------------------------------------------
        [DllImport(Lib)] internal static extern int pf_engine_create(ref PfEngineConfig cfg, out IntPtr engine);
        [DllImport(Lib)] internal static extern void pf_engine_destroy(IntPtr engine);
        [DllImport(Lib)] internal static extern int pf_engine_info(IntPtr e, out int kind, out int vocab, out int featDim, out int hasTs);
        [DllImport(Lib)] internal static extern int pf_frontend_num_frames(IntPtr e, long nSamples, out int tLfr);
        [DllImport(Lib)] internal static extern int pf_frontend(IntPtr e, float[] samples, long n, [Out] float[] feats, long featsCap, out int tLfr);
        [DllImport(Lib)] internal static extern int pf_fbank(IntPtr e, float[] samples, long n, [Out] float[] fbank, long cap, out int t80);
        [DllImport(Lib)] internal static extern int pf_model_proj(IntPtr e, IntPtr[] speech, int[] speechLenFloats, int B,
                                                                 int[]? hotwords, int nHotwords, ref PfBatchOut o);
        [DllImport(Lib)] internal static extern int pf_forward_feats(IntPtr e, float[] speech, int B, int tMax,
                                                                    int[]? hotwords, int nHotwords, ref PfBatchOut o);
        [DllImport(Lib)] internal static extern int pf_recognize(IntPtr e, IntPtr[] samples, long[] nSamples, int B,
                                                                int[]? hotwords, int nHotwords, ref PfBatchOut o);
        [DllImport(Lib)] internal static extern int pf_fetch(IntPtr e, ref PfBatchOut o);
        [DllImport(Lib)] internal static extern int pf_fetch_ids_device(IntPtr e, IntPtr idsDev, int lCap, out int L);
        // decoding extras (additions to ABI 6): PF_DECODE_SCORES = 1, PF_DECODE_CTC = 2 (CTC collapse with per-token first /
        // last frame and score, SenseVoice); fetch them BEFORE the pf_fetch that receives token_ids
        internal const int PF_DECODE_SCORES = 1, PF_DECODE_CTC = 2;
        [DllImport(Lib)] internal static extern int pf_engine_set_decode(IntPtr e, int flags);
        [DllImport(Lib)] internal static extern int pf_fetch_scores(IntPtr e, [Out] float[]? scores, long cap, out int L);
        [DllImport(Lib)] internal static extern int pf_fetch_ctc(IntPtr e, [Out] long[]? ids, [Out] int[]? first, [Out] int[]? last,
                                                                [Out] float[]? score, int cap, [Out] int[]? n, out int nMax);
        // top-k and n-best (additions to ABI 6): PF_DECODE_TOPK keeps the K (1 .. PF_TOPK_MAX, default 4) best (id, log-prob)
        // pairs of every position, larger value first and of equal values the larger id; pf_host_nbest turns one utterance's
        // lists into its exact N-best rank vectors (N <= PF_NBEST_MAX)
        internal const int PF_DECODE_TOPK = 8, PF_TOPK_MAX = 8, PF_NBEST_MAX = 64;
        [DllImport(Lib)] internal static extern int pf_engine_set_topk(IntPtr e, int k);
        [DllImport(Lib)] internal static extern int pf_fetch_topk(IntPtr e, [Out] long[]? ids, [Out] float[]? val, [Out] int[]? n, long capRows,
                                                                 out int L, out int K);
        // CTC beam search (additions to ABI 6): PF_DECODE_CTC_BEAM (SenseVoice; implies TOPK and SCORES) keeps the N best labelings
        // of a prefix beam search of width W (1 <= N <= W <= PF_NBEST_MAX, default 16 / 16) with their float64 scores
        internal const int PF_DECODE_CTC_BEAM = 16;
        [DllImport(Lib)] internal static extern int pf_engine_set_ctc_beam(IntPtr e, int W, int N);
        [DllImport(Lib)] internal static extern int pf_fetch_ctc_beam(IntPtr e, [Out] long[]? ids, [Out] int[]? len, [Out] double[]? score, int cap,
                                                                     [Out] int[]? nHyp, out int lenMax);
        [DllImport(Lib)] internal static extern int pf_host_ctc_beam(float[] blankLp, long blankStride, long[] ids, float[] val, int[] n, int T, int K,
                                                                    int blank, int W, int N, [Out] long[] outIds, [Out] int[] outLen,
                                                                    [Out] double[] outScore, int cap, out int nHyp);
        // CTC hot words (additions to ABI 6): a hot-word set and a boost per matched token inside the beam search (SenseVoice); with a
        // set installed PF_DECODE_CTC_BEAM runs the biased search: score = loglik_sum + boost * matched, in the biased order
        internal const int PF_HOTWORD_STATES_MAX = 4096, PF_HOTWORD_LEN_MAX = 64, PF_HOTWORD_TABLE_BYTES_MAX = 16 * 1024 * 1024;
        [DllImport(Lib)] internal static extern int pf_host_hotword_graph(int[]? ids, int[]? lens, int nHotwords, int V, out int nStates, out int nCols,
                                                                         [Out] int[]? tokCol, [Out] int[]? table, long tableCap,
                                                                         [Out] int[]? depth, int depthCap);
        [DllImport(Lib)] internal static extern int pf_engine_set_ctc_hotwords(IntPtr e, int[]? ids, int[]? lens, int nHotwords, float boost);
        [DllImport(Lib)] internal static extern int pf_fetch_ctc_beam_hot(IntPtr e, [Out] int[]? matched, [Out] double[]? loglikSum);
        [DllImport(Lib)] internal static extern int pf_host_ctc_beam_hot(float[] blankLp, long blankStride, long[] ids, float[] val, int[] n, int T, int K,
                                                                        int blank, int W, int N, [Out] long[] outIds, [Out] int[] outLen,
                                                                        [Out] double[] outScore, int cap, out int nHyp, int[]? hwIds, int[]? hwLens,
                                                                        int nHotwords, float boost, [Out] int[] outMatched, [Out] double[] outLoglik);
        [DllImport(Lib)] internal static extern int pf_op_ctc_beam_hot(IntPtr e, float[] blankLp, long[] ids, float[] val, int[] n, int[] lens, int B,
                                                                      int T, int K, int blank, int W, int N, [Out] long[] outIds, [Out] int[] outLen,
                                                                      [Out] double[] outScore, int cap, [Out] int[] nHyp, int[]? hwIds, int[]? hwLens,
                                                                      int nHotwords, float boost, [Out] int[] outMatched, [Out] double[] outLoglik);
        // CTC language model (additions to ABI 6): a back-off n-gram LM compiled on the host (pf_lm handle), its plain walk, and
        // the fused forms of the beam search
        internal const int PF_LM_ORDER_MAX = 8, PF_LM_IMAGE_BYTES_MAX = 1024 * 1024 * 1024, PF_LM_EOS = 1;
        [DllImport(Lib)] internal static extern int pf_host_lm_build(int order, long[] nNgrams, int[]? ids, float[]? logp, float[]? backoff, int V, int bos,
                                                                    int eos, int unk, float oov, int[]? transparent, int nTransparent, out IntPtr lm);
        [DllImport(Lib)] internal static extern int pf_host_lm_from_arpa([MarshalAs(UnmanagedType.LPUTF8Str)] string path, IntPtr[] tokens, int nTokens,
                                                                        float oov, out long nDropped, out IntPtr lm);
        [DllImport(Lib)] internal static extern int pf_host_lm_info(IntPtr lm, out int order, out long nStates, out long nArcs, out long imageBytes);
        [DllImport(Lib)] internal static extern int pf_host_lm_score(IntPtr lm, int[]? ids, int n, float alpha, float beta, int flags, out double g,
                                                                    out int state, [Out] double[]? gPos, [Out] int[]? statePos);
        [DllImport(Lib)] internal static extern void pf_lm_free(IntPtr lm);
        [DllImport(Lib)] internal static extern int pf_engine_set_ctc_lm(IntPtr e, IntPtr lm, float alpha, float beta, int flags);
        [DllImport(Lib)] internal static extern int pf_fetch_ctc_beam_lm(IntPtr e, [Out] double[]? lmSum, [Out] double[]? loglikSum);
        [DllImport(Lib)] internal static extern int pf_host_ctc_beam_lm(float[] blankLp, long blankStride, long[] ids, float[] val, int[] n, int T, int K,
                                                                       int blank, int W, int N, [Out] long[] outIds, [Out] int[] outLen,
                                                                       [Out] double[] outScore, int cap, out int nHyp, int[]? hwIds, int[]? hwLens,
                                                                       int nHotwords, float boost, [Out] int[] outMatched, [Out] double[] outLoglik,
                                                                       IntPtr lm, float alpha, float beta, int flags, [Out] double[] outLm);
        // N-best search (additions to ABI 6): a paraformer's position-synchronous beam search over its top-k lists on the device,
        // optionally fused with a hot-word set and the n-gram LM above; with a search installed a forward with PF_DECODE_TOPK runs it
        [DllImport(Lib)] internal static extern int pf_engine_set_nbest_search(IntPtr e, int W, int N);
        [DllImport(Lib)] internal static extern int pf_engine_set_nbest_lm(IntPtr e, IntPtr lm, float alpha, float beta, int flags);
        [DllImport(Lib)] internal static extern int pf_engine_set_nbest_hotwords(IntPtr e, int[]? ids, int[]? lens, int nHotwords, float boost);
        [DllImport(Lib)] internal static extern int pf_fetch_nbest_search(IntPtr e, [Out] int[]? ranks, [Out] double[]? score, [Out] double[]? loglikSum,
                                                                         [Out] double[]? lmSum, [Out] int[]? matched, [Out] int[]? nHyp, out int L,
                                                                         out int N);
        [DllImport(Lib)] internal static extern int pf_host_nbest_search(long[] ids, float[] val, int[] n, int L, int K, int tokenNum, int W, int N,
                                                                        int[]? hwIds, int[]? hwLens, int nHotwords, float boost, IntPtr lm,
                                                                        float alpha, float beta, int flags, [Out] int[] outRanks,
                                                                        [Out] double[]? outScore, [Out] double[]? outLoglik, [Out] double[]? outLm,
                                                                        [Out] int[]? outMatched, out int nHyp);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_nbest_search(IntPtr r, int W);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_nbest_lm(IntPtr r, [MarshalAs(UnmanagedType.LPUTF8Str)] string? arpaPath, float alpha,
                                                                              float beta, int flags);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_nbest_hotword_boost(IntPtr r, float boost);
        [DllImport(Lib)] internal static extern int pf_op_ctc_beam_lm(IntPtr e, float[] blankLp, long[] ids, float[] val, int[] n, int[] lens, int B,
                                                                     int T, int K, int blank, int W, int N, [Out] long[] outIds, [Out] int[] outLen,
                                                                     [Out] double[] outScore, int cap, [Out] int[] nHyp, int[]? hwIds, int[]? hwLens,
                                                                     int nHotwords, float boost, [Out] int[] outMatched, [Out] double[] outLoglik,
                                                                     IntPtr lm, float alpha, float beta, int flags, [Out] double[] outLm);
        [DllImport(Lib)] internal static extern int pf_op_lm_score(IntPtr e, IntPtr lm, int[] ids, int[] lens, int B, int L, float alpha, float beta,
                                                                  [Out] double[] g, [Out] int[] state);
        // The int8 path (math_mode 2) one kernel at a time, for parity tests: the activation quantiser (optionally behind a
        // LayerNorm that is never stored), the weight quantiser, the import of an export's stored bytes, and the integer GEMM on
        // codes and parameters as given.  Hostile hosts: PF_ERR_DEVICE when a result cell comes back unwritten or a kernel stored
        // outside what its contract allows.  codes / w: signed bytes (code - 128), pad columns included.
        [StructLayout(LayoutKind.Sequential)]
        internal struct PfQgemmDesc
        {
            public int struct_size, M, N, K, relu, out_kind, tile_rows, want_range, scale_cols;
            public float scale, a_scale;
            public int a_zp;
            public IntPtr w_zp, w_scale, bias, resid, add2;
        }
        [DllImport(Lib)] internal static extern int pf_op_quantize(IntPtr e, float[] x, int rows, int cols, int ldx, int xIsF16, int ld, float[]? gamma,
                                                                  float[]? beta, [Out] sbyte[] codes, [Out] int[] rowsum, [Out] float[] scaleZp);
        [DllImport(Lib)] internal static extern int pf_op_quantize_weight(IntPtr e, float[] W, int N, int K, int ld, [Out] sbyte[] w, [Out] int[] colsum,
                                                                         [Out] int[] wzp, [Out] float[] wscale, [Out] int[] dz);
        [DllImport(Lib)] internal static extern int pf_op_import_weight(IntPtr e, byte[] Q, byte[] zp, float[] scale, int N, int K, int ld, [Out] sbyte[] w,
                                                                       [Out] int[] colsum, [Out] int[] wzp, [Out] float[] wscale, [Out] int[] dz);
        [DllImport(Lib)] internal static extern int pf_op_qgemm_ex(IntPtr e, ref PfQgemmDesc d, byte[] aCodes, byte[] wCodes, [Out] float[]? y32,
                                                                  [Out] float[]? y16, [Out] float[]? range);
        // CTC forced alignment (additions to ABI 6): PF_DECODE_ALIGN (SenseVoice; implies SCORES) aligns the targets set for the next
        // forward, and with PF_DECODE_CTC_BEAM the beam's hypotheses, to the log-prob rows: Viterbi path and log-likelihood per job
        internal const int PF_DECODE_ALIGN = 32;
        internal const int PF_ALIGN_MAX_TOKENS = 1023;
        [DllImport(Lib)] internal static extern int pf_engine_set_align_targets(IntPtr e, long[]? ids, int[]? len, int B, int cap);
        [DllImport(Lib)] internal static extern int pf_fetch_align(IntPtr e, [Out] float[]? pathScore, [Out] double[]? loglik, [Out] int[]? ok,
                                                                  [Out] int[]? len, [Out] int[]? first, [Out] int[]? last,
                                                                  [Out] float[]? tokScore, int cap, out int H, out int lenMax);
        [DllImport(Lib)] internal static extern int pf_host_ctc_align(float[] lp, long ld, int T, int V, long[] y, int U, out float pathScore,
                                                                     out double loglik, out int ok, [Out] int[] first, [Out] int[] last,
                                                                     [Out] float[] tokScore);
        [DllImport(Lib)] internal static extern int pf_host_nbest(long[]? ids, float[] val, int[] n, int L, int K, int nFree, int N,
                                                                 [Out] int[] outRanks, [Out] double[] outScores, out int nOut);

        // PCM intake (additions to ABI 6): raw interleaved values, decoded / down-mixed / resampled on the device in front of the
        // fbank, bit for bit what GetFileSample (Examples/Utils/AudioHelper.cs:12-32) returns; nValues counts interleaved values
        internal const int PF_PCM_U8 = 1, PF_PCM_S16 = 2, PF_PCM_S24 = 3, PF_PCM_S32 = 4, PF_PCM_F32 = 5, PF_PCM_F64 = 6, PF_PCM_ALAW = 7,
                           PF_PCM_MULAW = 8, PF_PCM_DOWNMIX_ALWAYS = 1;
        [DllImport(Lib)] internal static extern int pf_pcm_num_samples(ref PfPcmDesc desc, int fs, long nValues, out long nOut);
        [DllImport(Lib)] internal static extern int pf_stage_pcm(IntPtr e, IntPtr[] data, long[] nValues, PfPcmDesc[] descs, int nDescs, int B);
        [DllImport(Lib)] internal static extern int pf_recognize_pcm(IntPtr e, IntPtr[] data, long[] nValues, PfPcmDesc[] descs, int nDescs,
                                                                    int B, int[]? hotwords, int nHotwords, ref PfBatchOut o);

        // ---- several GPUs in one process (paraformer_hip.h section 4b) ------------------------------------------
        [DllImport(Lib)] internal static extern int pf_group_create(ref PfEngineConfig cfg, int[] devices, int nDevices, out IntPtr group);
        [DllImport(Lib)] internal static extern void pf_group_destroy(IntPtr group);
        [DllImport(Lib)] internal static extern int pf_group_info(IntPtr g, out int nEngines, out int usesRccl);
        [DllImport(Lib)] internal static extern int pf_group_recognize(IntPtr g, IntPtr[] samples, long[] nSamples, int B,
                                                                      int[]? hotwords, int nHotwords, ref PfBatchOut o);
        [DllImport(Lib)] internal static extern int pf_group_fetch(IntPtr g, ref PfBatchOut o);
        /// <summary>Host-only rehearsal of pf_group_recognize's shard plan / rendez-vous / merge (no GPU): see paraformer_hip.h.</summary>
        [DllImport(Lib)] internal static extern int pf_host_group_sim(int G, int B, int[] fireCount, int hasCif, int fixedL, int collective,
                                                                     int failShard, int failStage, [Out] long[] idsOut, int lCap,
                                                                     [Out] int[] tokenNumOut, out int L);

        // ---- profiling (bench harness) ---------------------------------------------------------------------------
        [DllImport(Lib)] internal static extern int pf_profile_enable(IntPtr e, int on);
        [DllImport(Lib)] internal static extern int pf_profile_reset(IntPtr e);
        [DllImport(Lib, CharSet = CharSet.Ansi)] internal static extern int pf_profile_select(IntPtr e, string? className);
        [DllImport(Lib, CharSet = CharSet.Ansi)] internal static extern int pf_profile_get(IntPtr e, string className, out double totalMs, out long launches, out double flopsPerLaunch);
        [DllImport(Lib, CharSet = CharSet.Ansi)] internal static extern int pf_profile_kernel(IntPtr e, string className, [Out] byte[] nameOut, int cap);

        // ---- whole-class mirror (OfflineRecognizer / OfflineStream) ---------------------------------------------
        [DllImport(Lib, CharSet = CharSet.Ansi)]
        internal static extern int pf_recognizer_create([MarshalAs(UnmanagedType.LPUTF8Str)] string model,
            [MarshalAs(UnmanagedType.LPUTF8Str)] string config, [MarshalAs(UnmanagedType.LPUTF8Str)] string mvn,
            [MarshalAs(UnmanagedType.LPUTF8Str)] string tokens, [MarshalAs(UnmanagedType.LPUTF8Str)] string modeleb,
            [MarshalAs(UnmanagedType.LPUTF8Str)] string hotword, int batchSize, int threadsNum, int device, out IntPtr recognizer);
        [DllImport(Lib)] internal static extern void pf_recognizer_dispose(IntPtr r);
        [DllImport(Lib)] internal static extern void pf_recognizer_free(IntPtr r);
        [DllImport(Lib)] internal static extern int pf_recognizer_num_engines(IntPtr r);   // engines of the pool ($PF_RECOGNIZER_ENGINES)
        [DllImport(Lib)] internal static extern int pf_recognizer_create_stream(IntPtr r, out IntPtr stream);
        [DllImport(Lib)] internal static extern int pf_stream_add_samples(IntPtr s, float[]? samples, long n);
        [DllImport(Lib)] internal static extern int pf_stream_add_pcm(IntPtr s, byte[]? data, long nValues, ref PfPcmDesc desc);
        [DllImport(Lib)] internal static extern int pf_stream_add_pcm(IntPtr s, short[]? data, long nValues, ref PfPcmDesc desc);
        [DllImport(Lib)] internal static extern int pf_stream_set_hotwords(IntPtr s, int[]? ids, int[]? lens, int nHotwords);
        [DllImport(Lib)] internal static extern int pf_stream_get_hotwords(IntPtr s, [Out] int[] ids, int idsCap, [Out] int[] lens, int lensCap, out int nHotwords);
        [DllImport(Lib)] internal static extern int pf_stream_num_feature_floats(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_stream_tokens(IntPtr s, out IntPtr ids, out int n);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_decode(IntPtr r, int flags);
        [DllImport(Lib)] internal static extern int pf_stream_scores(IntPtr s, out IntPtr scores, out int n);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_nbest(IntPtr r, int N, int K);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_ctc_beam(IntPtr r, int N, int W, int K);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_align(IntPtr r, int on);
        [DllImport(Lib)] internal static extern int pf_stream_set_align_ids(IntPtr s, long[]? ids, int n);
        [DllImport(Lib)] internal static extern int pf_stream_alignment(IntPtr s, out IntPtr beginEnd, out IntPtr tokScore, out int n, out float pathScore,
                                                                       out double loglik, out int ok);
        [DllImport(Lib)] internal static extern int pf_stream_alternative_timestamps(IntPtr s, int i, out IntPtr beginEnd, out int n, out double loglik);
        // long-audio recognition: voice-activity segmentation on the device, batches of similar length, one result per stream
        [DllImport(Lib)] internal static extern int pf_vad_default(out PfVadConfig cfg);
        [DllImport(Lib)] internal static extern int pf_endpoint_default(out PfEndpointConfig cfg);
        // the FSMN-VAD model score (a .pfw of kind "fsmnvad"): the loader, what it read, the defaults that go with it, the attach calls
        [DllImport(Lib)] internal static extern int pf_vad_model_load([MarshalAs(UnmanagedType.LPUTF8Str)] string path, out IntPtr m);
        [DllImport(Lib)] internal static extern int pf_vad_model_from_memory(byte[] data, long nbytes, out IntPtr m);
        [DllImport(Lib)] internal static extern int pf_vad_model_info(IntPtr m, [Out] int[]? dims, out int nSil, out long imageBytes);
        [DllImport(Lib)] internal static extern int pf_vad_model_sil_ids(IntPtr m, [Out] int[]? sil, int cap, out int n);
        [DllImport(Lib)] internal static extern int pf_vad_model_tensor(IntPtr m, [MarshalAs(UnmanagedType.LPUTF8Str)] string name, [Out] float[]? data,
                                                                       long cap, out long n);
        [DllImport(Lib)] internal static extern int pf_vad_model_config(out PfVadConfig cfg);
        [DllImport(Lib)] internal static extern int pf_endpoint_model_config(out PfEndpointConfig cfg);
        [DllImport(Lib)] internal static extern int pf_vad_model_stream_state_bytes(IntPtr m, out long bytes);
        [DllImport(Lib)] internal static extern int pf_punc_model_causal(IntPtr m, out int causal);
        [DllImport(Lib)] internal static extern int pf_punc_stream_state_bytes(IntPtr m, out long bytes);
        [DllImport(Lib)] internal static extern int pf_online_recognizer_set_punc_model(IntPtr r, [MarshalAs(UnmanagedType.LPUTF8Str)] string? pfwPath, int maxContext);
        [DllImport(Lib)] internal static extern int pf_online_stream_punctuated(IntPtr s, out IntPtr textUtf8, out IntPtr puncIds, out IntPtr puncFlags, out int nWords);
        [DllImport(Lib)] internal static extern int pf_online_stream_sentence_punctuated(IntPtr s, int j, out IntPtr textUtf8, out IntPtr puncIds, out int nWords);
        [DllImport(Lib)] internal static extern void pf_vad_model_free(IntPtr m);
        [DllImport(Lib)] internal static extern int pf_engine_set_vad_model(IntPtr e, IntPtr m);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_vad_model(IntPtr r, [MarshalAs(UnmanagedType.LPUTF8Str)] string? pfwPath);
        [DllImport(Lib)] internal static extern int pf_vad_segment(IntPtr e, IntPtr[] samples, long[] nSamples, int B, ref PfVadConfig cfg,
                                                                  [Out] int[] seg, int cap, [Out] int[] nSeg);
        // cfg: an array of one element, or null (= off)
        [DllImport(Lib)] internal static extern int pf_recognizer_set_vad(IntPtr r, PfVadConfig[]? cfg, int batchMax, long frameBudget,
                                                                         [MarshalAs(UnmanagedType.LPUTF8Str)] string? sepUtf8);
        // punctuation (a .pfw of kind "cttransformer"): the loader, what it read, the attach calls, the loop on ids, a stream's result
        [DllImport(Lib)] internal static extern int pf_punc_model_load([MarshalAs(UnmanagedType.LPUTF8Str)] string path, out IntPtr m);
        [DllImport(Lib)] internal static extern int pf_punc_model_from_memory(byte[] data, long nbytes, out IntPtr m);
        [DllImport(Lib)] internal static extern int pf_punc_model_info(IntPtr m, [Out] int[]? dims, out long imageBytes);
        [DllImport(Lib)] internal static extern void pf_punc_model_free(IntPtr m);
        [DllImport(Lib)] internal static extern int pf_engine_set_punc_model(IntPtr e, IntPtr m);
        [DllImport(Lib)] internal static extern int pf_engine_punctuate(IntPtr e, int[] ids, int[] lens, int B, [Out] int[] puncIds, out int rounds);
        // speaker labels (a .pfw of kind "campplus"): the loader, what it read, the defaults, the attach calls, a stream's result
        [DllImport(Lib)] internal static extern int pf_spk_model_load([MarshalAs(UnmanagedType.LPUTF8Str)] string path, out IntPtr m);
        [DllImport(Lib)] internal static extern int pf_spk_model_from_memory(byte[] data, long nbytes, out IntPtr m);
        [DllImport(Lib)] internal static extern int pf_spk_model_info(IntPtr m, [Out] int[]? dims, out long imageBytes);
        [DllImport(Lib)] internal static extern void pf_spk_model_free(IntPtr m);
        [DllImport(Lib)] internal static extern int pf_spk_default(out PfSpkConfig cfg);
        [DllImport(Lib)] internal static extern int pf_engine_set_spk_model(IntPtr e, IntPtr m);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_spk_model(IntPtr r, [MarshalAs(UnmanagedType.LPUTF8Str)] string? pfwPath, ref PfSpkConfig cfg);
        [DllImport(Lib)] internal static extern int pf_stream_num_speakers(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_stream_segment_speaker(IntPtr s, int i, out int spk);
        [DllImport(Lib)] internal static extern int pf_stream_speaker_centroid(IntPtr s, int spk, [Out] float[]? centroid, int cap, out int e);
        [DllImport(Lib)] internal static extern int pf_stream_num_spk_windows(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_stream_spk_window(IntPtr s, int i, out int beginMs, out int endMs, out int label);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_punc_model(IntPtr r, [MarshalAs(UnmanagedType.LPUTF8Str)] string? pfwPath);
        [DllImport(Lib)] internal static extern int pf_stream_punctuated(IntPtr s, out IntPtr textUtf8, out IntPtr puncIds, out int nWords);
        [DllImport(Lib)] internal static extern int pf_stream_num_sentences(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_stream_sentence(IntPtr s, int i, out int wordBegin, out int wordEnd, out int hasTime,
                                                                      out int beginMs, out int endMs, out IntPtr textUtf8);
        [DllImport(Lib)] internal static extern int pf_stream_num_segments(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_stream_segment(IntPtr s, int i, out int beginMs, out int endMs, out int batch, out int row,
                                                                     out int tokBegin, out int tokEnd, out IntPtr textUtf8);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_hotword_boost(IntPtr r, float boost);
        [DllImport(Lib)] internal static extern int pf_stream_alternative_hot(IntPtr s, int i, out int hotwordTokens, out double loglikSum);
        [DllImport(Lib)] internal static extern int pf_recognizer_set_lm(IntPtr r, [MarshalAs(UnmanagedType.LPUTF8Str)] string? arpaPath, float alpha,
                                                                        float beta, int flags);
        [DllImport(Lib)] internal static extern int pf_stream_alternative_lm(IntPtr s, int i, out double lmSum, out double loglikSum);
        [DllImport(Lib)] internal static extern int pf_stream_token_alternatives(IntPtr s, out IntPtr ids, out IntPtr val, out int nTokens, out int K);
        [DllImport(Lib)] internal static extern int pf_stream_num_alternatives(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_stream_alternative(IntPtr s, int i, out IntPtr ids, out int nIds, out double score,
                                                                         out IntPtr textUtf8, out int nTokens);
        [DllImport(Lib)] internal static extern int pf_stream_alternative_token(IntPtr s, int i, int j, out IntPtr utf8);
        // ABI 6: the rest of OfflineStream's public surface (OfflineStream.cs:20-34)
        [DllImport(Lib)] internal static extern int pf_stream_create([MarshalAs(UnmanagedType.LPUTF8Str)] string mvnPath, int fs, int nMels, int lfrM, int lfrN,
                                                                    int snipEdges, float dither, [MarshalAs(UnmanagedType.LPUTF8Str)] string window, out IntPtr stream);
        [DllImport(Lib)] internal static extern int pf_stream_set_tokens(IntPtr s, long[]? ids, int n);
        [DllImport(Lib)] internal static extern int pf_stream_num_timestamps(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_stream_timestamp(IntPtr s, int j, out IntPtr ints, out int nInts);
        [DllImport(Lib)] internal static extern int pf_stream_set_timestamps(IntPtr s, int[]? ints, int[]? lens, int n);
        [DllImport(Lib)] internal static extern int pf_stream_get_speech(IntPtr s, [Out] float[]? speech, long cap, out int nFloats);
        [DllImport(Lib)] internal static extern int pf_stream_set_speech(IntPtr s, float[]? speech, int nFloats, int speechLength);
        [DllImport(Lib)] internal static extern void pf_stream_dispose(IntPtr s);
        [DllImport(Lib)] internal static extern void pf_stream_free(IntPtr s);
        [DllImport(Lib)] internal static extern int pf_recognizer_get_results(IntPtr r, IntPtr[] streams, int nStreams);
        [DllImport(Lib)] internal static extern int pf_result_text(IntPtr r, int i, out IntPtr utf8, out int textLenUtf16);
        [DllImport(Lib)] internal static extern int pf_result_num_tokens(IntPtr r, int i, out int n);
        [DllImport(Lib)] internal static extern int pf_result_token(IntPtr r, int i, int j, out IntPtr utf8);
        [DllImport(Lib)] internal static extern int pf_result_num_timestamps(IntPtr r, int i, out int n);
        [DllImport(Lib)] internal static extern int pf_result_timestamp(IntPtr r, int i, int j, out IntPtr ints, out int nInts);

        /// <summary>pf_status -> the exception the reference throws at the same place (INTEGRATION.md section 1).</summary>
        internal static void Check(int rc)
        {
            if (rc >= 0) return;
            string msg = Marshal.PtrToStringUTF8(pf_last_error()) ?? "";
            switch (rc)
            {
                case PF_ERR_TOKENS: throw new Exception("tokens invalid");                        // OfflineRecognizer.cs:32
                case PF_ERR_DISPOSED: throw new ObjectDisposedException(msg.Length > 0 ? msg : "OfflineRecognizer");   // :96
                case PF_ERR_NULL_SAMPLES: throw new ArgumentNullException("source");              // WavFrontend.cs:34
                case PF_ERR_RECOGNITION: throw new Exception("Offline recognition failed", new Exception(msg));   // :194-197
                default: throw new Exception(msg);
            }
        }
    }
}
