// OfflineRecognizerHip.cs — drop-in classes with the public signatures of OfflineRecognizer
// (AliParaformerAsr/OfflineRecognizer.cs:23,92,102,110,441,468) and OfflineStream (OfflineStream.cs:20,30-34,36,58,69,115), backed
// by the native mirror pf_recognizer_* / pf_stream_*: front-end, model, arg-max, time_stamp_lfr6_onnx and
// DecodeMulti all run behind the C ABI; only ids, timestamps and text cross it.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using AliParaformerAsr.Model;
using AliParaformerAsr.Native;

namespace AliParaformerAsr.Hip
{
    public class OfflineStream : IDisposable
    {
        internal IntPtr Handle;
        internal OfflineStream(IntPtr h) { Handle = h; }

        /// <summary>OfflineStream.cs:20-28.  A stream that belongs to no recognizer yet: its AddSamples calls are kept and
        /// replayed by the first GetResults that receives it (the front-end runs on that recognizer's GPU); the am.mvn values
        /// and frontend_conf must be that recognizer's.</summary>
        public OfflineStream(string mvnFilePath, ConfEntity confEntity)
        {
            FrontendConfEntity f = confEntity.frontend_conf;
            ParaformerHip.Check(ParaformerHip.pf_stream_create(mvnFilePath ?? "", f.fs, f.n_mels, f.lfr_m, f.lfr_n, f.snip_edges ? 1 : 0,
                                                               f.dither, f.window ?? "", out Handle));
        }

        public void AddSamples(float[] samples)
            => ParaformerHip.Check(ParaformerHip.pf_stream_add_samples(Handle, samples, samples == null ? 0 : samples.LongLength));

        /// <summary>Not in the reference: AddSamples for audio as a caller holds it — raw interleaved PCM of `format`
        /// (ParaformerHip.PF_PCM_*) at any rate, mono or stereo.  Decoded, down-mixed and resampled to the model's rate exactly
        /// as the Examples' GetFileSample does (a stereo stream AT the model's rate stays interleaved unless downmixAlways), on
        /// the device for the first call on a recognizer's stream.</summary>
        public void AddPcm(byte[] data, int sampleRate, int channels, int format = ParaformerHip.PF_PCM_S16, bool downmixAlways = false)
        {
            PfPcmDesc d = PfPcmDesc.Of(format, sampleRate, channels, downmixAlways);
            int bytesPerValue = format == ParaformerHip.PF_PCM_S16 ? 2 : format == ParaformerHip.PF_PCM_S24 ? 3
                              : format == ParaformerHip.PF_PCM_S32 || format == ParaformerHip.PF_PCM_F32 ? 4 : format == ParaformerHip.PF_PCM_F64 ? 8 : 1;
            ParaformerHip.Check(ParaformerHip.pf_stream_add_pcm(Handle, data, data == null ? 0 : data.LongLength / bytesPerValue, ref d));
        }

        /// <summary>16-bit PCM as most capture APIs deliver it.</summary>
        public void AddPcm(short[] samples, int sampleRate, int channels = 1, bool downmixAlways = false)
        {
            PfPcmDesc d = PfPcmDesc.Of(ParaformerHip.PF_PCM_S16, sampleRate, channels, downmixAlways);
            ParaformerHip.Check(ParaformerHip.pf_stream_add_pcm(Handle, samples, samples == null ? 0 : samples.LongLength, ref d));
        }

        /// <summary>OfflineStream.cs:58-68: the entity Forward reads.  A snapshot: features that live on the device are
        /// computed and read back for it.</summary>
        public OfflineInputEntity GetDecodeChunk() => OfflineInputEntity;

        /// <summary>OfflineStream.cs:69-79.</summary>
        public void RemoveChunk()
        {
            if (Tokens.Count > 2) ParaformerHip.Check(ParaformerHip.pf_stream_set_speech(Handle, null, -1, 0));
        }

        /// <summary>OfflineStream.cs:30.  get: a snapshot {Speech, SpeechLength, Hotwords}; set: written through.</summary>
        public OfflineInputEntity OfflineInputEntity
        {
            get
            {
                var e = new OfflineInputEntity();
                ParaformerHip.Check(ParaformerHip.pf_stream_num_feature_floats(Handle, out int len));
                int rc = ParaformerHip.pf_stream_get_speech(Handle, null, 0, out int n);
                if (rc == ParaformerHip.PF_ERR_CAPACITY)
                {
                    var a = new float[n];
                    ParaformerHip.Check(ParaformerHip.pf_stream_get_speech(Handle, a, a.LongLength, out n));
                    e.Speech = a;
                }
                else
                {
                    ParaformerHip.Check(rc);
                    e.Speech = n < 0 ? null : new float[0];
                }
                e.SpeechLength = len;
                e.Hotwords = Hotwords;
                return e;
            }
            set
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_set_speech(Handle, value?.Speech, value?.Speech == null ? -1 : value.Speech.Length,
                                                                       value?.SpeechLength ?? 0));
                Hotwords = value?.Hotwords;
            }
        }

        /// <summary>OfflineStream.cs:31.  {blank, blank} from the constructor on; nothing in the reference reads it afterwards
        /// (Forward works on Tokens), so it stays a managed field.</summary>
        public Int64[] Hyp { get; set; } = new Int64[] { 0, 0 };

        public List<int[]>? Hotwords
        {
            get
            {
                var ids = new int[4096]; var lens = new int[1024];
                ParaformerHip.Check(ParaformerHip.pf_stream_get_hotwords(Handle, ids, ids.Length, lens, lens.Length, out int n));
                if (n < 0) return null;
                var r = new List<int[]>(); int off = 0;
                for (int i = 0; i < n; i++) { r.Add(ids[off..(off + lens[i])]); off += lens[i]; }
                return r;
            }
            set
            {
                if (value == null) { ParaformerHip.Check(ParaformerHip.pf_stream_set_hotwords(Handle, null, null, -1)); return; }
                var flat = new List<int>(); var lens = new int[Math.Max(value.Count, 1)];
                for (int i = 0; i < value.Count; i++) { flat.AddRange(value[i]); lens[i] = value[i].Length; }
                ParaformerHip.Check(ParaformerHip.pf_stream_set_hotwords(Handle, flat.ToArray(), lens, value.Count));
            }
        }

        public List<Int64> Tokens
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_tokens(Handle, out IntPtr p, out int n));
                var a = new long[n];
                if (n > 0) Marshal.Copy(p, a, 0, n);
                return new List<Int64>(a);
            }
            set
            {
                long[] a = value == null ? new long[0] : value.ToArray();
                ParaformerHip.Check(ParaformerHip.pf_stream_set_tokens(Handle, a, a.Length));
            }
        }

        /// <summary>Not in the reference: scores (log-probs) of the last GetResults, parallel to Tokens — token confidences
        /// after OfflineRecognizer.SetDecode(ctc: true), per-position values after SetDecode(scores: true), else empty.</summary>
        public List<float> Scores
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_scores(Handle, out IntPtr p, out int n));
                var a = new float[n];
                if (n > 0) Marshal.Copy(p, a, 0, n);
                return new List<float>(a);
            }
        }

        /// <summary>Not in the reference: per entry of Tokens the K best (id, log-prob) pairs of the last GetResults, best first
        /// (OfflineRecognizer.SetNBest; empty without it).  Slots a position could not fill hold (-1, -inf).</summary>
        public List<(long Id, float LogProb)[]> TokenAlternatives
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_token_alternatives(Handle, out IntPtr pi, out IntPtr pv, out int n, out int k));
                var ids = new long[n * k]; var val = new float[n * k];
                if (n * k > 0) { Marshal.Copy(pi, ids, 0, n * k); Marshal.Copy(pv, val, 0, n * k); }
                var r = new List<(long, float)[]>(n);
                for (int t = 0; t < n; t++)
                {
                    var row = new (long, float)[k];
                    for (int j = 0; j < k; j++) row[j] = (ids[t * k + j], val[t * k + j]);
                    r.Add(row);
                }
                return r;
            }
        }

        /// <summary>Not in the reference: the n-best list of the last GetResults (paraformer models, SetNBest with N &gt; 1; else
        /// empty), by descending Score; entry 0 is the result itself.</summary>
        public List<Alternative> Alternatives
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_num_alternatives(Handle, out int n));
                var r = new List<Alternative>(n);
                for (int i = 0; i < n; i++)
                {
                    ParaformerHip.Check(ParaformerHip.pf_stream_alternative(Handle, i, out IntPtr p, out int k, out double score,
                                                                            out IntPtr txt, out int nt));
                    var a = new Alternative { Ids = new long[k], Score = score, Text = Marshal.PtrToStringUTF8(txt) ?? "" };
                    if (k > 0) Marshal.Copy(p, a.Ids, 0, k);
                    for (int j = 0; j < nt; j++)
                    {
                        ParaformerHip.Check(ParaformerHip.pf_stream_alternative_token(Handle, i, j, out IntPtr t));
                        a.Tokens.Add(Marshal.PtrToStringUTF8(t) ?? "");
                    }
                    ParaformerHip.Check(ParaformerHip.pf_stream_alternative_timestamps(Handle, i, out IntPtr pt, out int nts, out double ll));
                    var flat = new int[2 * nts];
                    if (nts > 0) Marshal.Copy(pt, flat, 0, 2 * nts);
                    for (int j = 0; j < nts; j++) a.Timestamps.Add(new[] { flat[2 * j], flat[2 * j + 1] });
                    a.LogLik = ll;
                    ParaformerHip.Check(ParaformerHip.pf_stream_alternative_hot(Handle, i, out int hot, out double llSum));
                    a.HotwordTokens = hot;
                    a.LogLikSum = llSum;
                    ParaformerHip.Check(ParaformerHip.pf_stream_alternative_lm(Handle, i, out double lmSum, out double _));
                    a.LmSum = lmSum;
                    r.Add(a);
                }
                return r;
            }
        }

        /// <summary>Not in the reference: one speech piece of a long stream (OfflineRecognizer.SetVad): [BeginMs, EndMs) on the
        /// stream's clock, where it ran in the call's batch plan, its share [TokBegin, TokEnd) of Tokens / Scores / Timestamps and
        /// its own text.</summary>
        public sealed class Segment
        {
            public int BeginMs, EndMs, Batch, Row, TokBegin, TokEnd;
            public string Text = "";
        }

        /// <summary>Not in the reference: the pieces the last GetResults cut this stream into, in time order (empty without
        /// OfflineRecognizer.SetVad).</summary>
        public List<Segment> Segments
        {
            get
            {
                var r = new List<Segment>();
                ParaformerHip.Check(ParaformerHip.pf_stream_num_segments(Handle, out int n));
                for (int i = 0; i < n; i++)
                {
                    ParaformerHip.Check(ParaformerHip.pf_stream_segment(Handle, i, out int b, out int e, out int batch, out int row, out int t0,
                                                                       out int t1, out IntPtr txt));
                    r.Add(new Segment { BeginMs = b, EndMs = e, Batch = batch, Row = row, TokBegin = t0, TokEnd = t1,
                                        Text = Marshal.PtrToStringUTF8(txt) ?? "" });
                }
                return r;
            }
        }

        /// <summary>Not in the reference: the speaker label of every entry of Segments (OfflineRecognizer.SetSpeakerModel with
        /// SetVad; empty without it): 0, 1, .. in the order of each speaker's first window, -1 when the stream has no window.</summary>
        public List<int> SegmentSpeakers
        {
            get
            {
                var r = new List<int>();
                ParaformerHip.Check(ParaformerHip.pf_stream_num_segments(Handle, out int n));
                ParaformerHip.Check(ParaformerHip.pf_stream_num_spk_windows(Handle, out int w));
                ParaformerHip.Check(ParaformerHip.pf_stream_num_speakers(Handle, out int k));
                if (w == 0 && k == 0) return r;
                for (int i = 0; i < n; i++)
                {
                    ParaformerHip.Check(ParaformerHip.pf_stream_segment_speaker(Handle, i, out int spk));
                    r.Add(spk);
                }
                return r;
            }
        }

        /// <summary>Not in the reference: speaker spk's centroid (pf_stream_speaker_centroid), for matching against enrolled voices.</summary>
        public float[] SpeakerCentroid(int spk)
        {
            ParaformerHip.Check(ParaformerHip.pf_stream_speaker_centroid(Handle, spk, null, 0, out int e));
            var c = new float[e];
            ParaformerHip.Check(ParaformerHip.pf_stream_speaker_centroid(Handle, spk, c, e, out e));
            return c;
        }

        /// <summary>Not in the reference: window i that was embedded, in ms, and its label (pf_stream_spk_window).</summary>
        public (int BeginMs, int EndMs, int Label) SpeakerWindow(int i)
        {
            ParaformerHip.Check(ParaformerHip.pf_stream_spk_window(Handle, i, out int b, out int e, out int l));
            return (b, e, l);
        }

        /// <summary>Not in the reference: one sentence of the punctuated text: the words [WordBegin, WordEnd), its text, and
        /// [BeginMs, EndMs] when the result has exactly one Timestamps entry per word (HasTime).</summary>
        public sealed class Sentence
        {
            public int WordBegin, WordEnd, BeginMs, EndMs;
            public bool HasTime;
            public string Text = "";
        }

        /// <summary>Not in the reference: the punctuated form of the last GetResults' Text (OfflineRecognizer.SetPuncModel; "" without it).</summary>
        public string Punctuated
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_punctuated(Handle, out IntPtr txt, out _, out _));
                return Marshal.PtrToStringUTF8(txt) ?? "";
            }
        }

        /// <summary>Not in the reference: the mark of every word of that text, as an index into the model's punc_list.</summary>
        public int[] PuncIds
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_punctuated(Handle, out _, out IntPtr ids, out int n));
                var r = new int[n];
                if (n > 0) Marshal.Copy(ids, r, 0, n);
                return r;
            }
        }

        /// <summary>Not in the reference: the sentences of the punctuated text.</summary>
        public List<Sentence> Sentences
        {
            get
            {
                var r = new List<Sentence>();
                ParaformerHip.Check(ParaformerHip.pf_stream_num_sentences(Handle, out int n));
                for (int i = 0; i < n; i++)
                {
                    ParaformerHip.Check(ParaformerHip.pf_stream_sentence(Handle, i, out int wb, out int we, out int ht, out int b, out int e,
                                                                        out IntPtr txt));
                    r.Add(new Sentence { WordBegin = wb, WordEnd = we, HasTime = ht != 0, BeginMs = b, EndMs = e,
                                         Text = Marshal.PtrToStringUTF8(txt) ?? "" });
                }
                return r;
            }
        }

        /// <summary>Not in the reference: the stream's target for forced alignment (OfflineRecognizer.SetAlign) as token IDS — text
        /// to ids needs the model's tokenizer and is the caller's.  Kept until cleared with null.</summary>
        public void SetAlignIds(long[]? ids)
            => ParaformerHip.Check(ParaformerHip.pf_stream_set_align_ids(Handle, ids, ids == null ? -1 : ids.Length));

        /// <summary>Not in the reference: the forced alignment of the target of the last GetResults; null when nothing was aligned
        /// for this stream.</summary>
        public Alignment? Alignment
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_alignment(Handle, out IntPtr pt, out IntPtr ps, out int n, out float path,
                                                                      out double ll, out int ok));
                if (n < 0) return null;
                var a = new Alignment { Ok = ok != 0, PathScore = path, LogLik = ll };
                int k = ok != 0 ? n : 0;
                var flat = new int[2 * k]; var sc = new float[k];
                if (k > 0) { Marshal.Copy(pt, flat, 0, 2 * k); Marshal.Copy(ps, sc, 0, k); }
                for (int j = 0; j < k; j++) a.Timestamps.Add(new[] { flat[2 * j], flat[2 * j + 1] });
                a.Scores.AddRange(sc);
                return a;
            }
        }

        public List<int[]> Timestamps                                           // OfflineStream.cs:33
        {
            get
            {
                ParaformerHip.Check(ParaformerHip.pf_stream_num_timestamps(Handle, out int n));
                var r = new List<int[]>(n);
                for (int j = 0; j < n; j++)
                {
                    ParaformerHip.Check(ParaformerHip.pf_stream_timestamp(Handle, j, out IntPtr p, out int k));
                    var a = new int[k];
                    if (k > 0) Marshal.Copy(p, a, 0, k);
                    r.Add(a);
                }
                return r;
            }
            set
            {
                var flat = new List<int>(); var lens = new int[Math.Max(value?.Count ?? 0, 1)];
                for (int i = 0; i < (value?.Count ?? 0); i++) { flat.AddRange(value![i]); lens[i] = value[i].Length; }
                ParaformerHip.Check(ParaformerHip.pf_stream_set_timestamps(Handle, flat.ToArray(), lens, value?.Count ?? 0));
            }
        }

        protected virtual void Dispose(bool disposing)                          // OfflineStream.cs:81-113
        {   // later calls answer ObjectDisposedException("OfflineStream"); the finaliser releases the handle
            if (Handle != IntPtr.Zero) ParaformerHip.pf_stream_dispose(Handle);
        }
        public void Dispose() => Dispose(disposing: true);                      // :115 (the finaliser is NOT suppressed: it frees the handle)
        ~OfflineStream() { if (Handle != IntPtr.Zero) { ParaformerHip.pf_stream_free(Handle); Handle = IntPtr.Zero; } }
    }

    /// <summary>One entry of OfflineStream.Alternatives: the ids of every position, Score = the sum of their log-probs, and the
    /// Text / Tokens DecodeMulti makes of them.</summary>
    public sealed class Alternative
    {
        public long[] Ids = new long[0];
        public double Score;
        public string Text = "";
        public List<string> Tokens = new List<string>();
        /// <summary>SetAlign beside SetCtcBeam: one [begin, end] pair in ms per id from the labeling's own forced alignment (empty
        /// without) and the log of the sum over all of its alignments (NaN without).</summary>
        public List<int[]> Timestamps = new List<int[]>();
        public double LogLik = double.NaN;
        /// <summary>SetHotwordBoost beside SetCtcBeam: the hot-word tokens the labeling completed (Score = LogLikSum + boost *
        /// HotwordTokens) and the unbiased log of the alignments the search summed (0 / NaN when the search ran unbiased).</summary>
        public int HotwordTokens;
        public double LogLikSum = double.NaN;
        /// <summary>SetLm beside SetCtcBeam: the weighted language-model score of the labeling, Score = (LogLikSum + boost *
        /// HotwordTokens) + LmSum (NaN when the search ran without a model; LogLikSum is then filled with or without hot words).</summary>
        public double LmSum = double.NaN;
    }

    /// <summary>OfflineStream.Alignment: where each id of a known text lies in the audio.  Ok = false: the target does not fit the
    /// audio; Timestamps / Scores are then empty.</summary>
    public sealed class Alignment
    {
        public bool Ok;
        public float PathScore;
        public double LogLik;
        public List<int[]> Timestamps = new List<int[]>();
        public List<float> Scores = new List<float>();
    }

    public sealed class OfflineRecognizer : IDisposable
    {
        private IntPtr _r;

        public OfflineRecognizer(string modelFilePath, string configFilePath, string mvnFilePath, string tokensFilePath,
                                 string modelebFilePath = "", string hotwordFilePath = "", int batchSize = 1, int threadsNum = 1,
                                 int device = 0)
            => ParaformerHip.Check(ParaformerHip.pf_recognizer_create(modelFilePath, configFilePath, mvnFilePath, tokensFilePath,
                                                                      modelebFilePath ?? "", hotwordFilePath ?? "", batchSize,
                                                                      threadsNum, device, out _r));

        /// <summary>Engines of this recognizer's pool (round 5).  GetResults holds no lock in the reference
        /// (OfflineRecognizer.cs:110-198), so a server calls it from several threads; here every call takes a free engine of the
        /// pool (same device, one copy of the weights) — created on demand up to $PF_RECOGNIZER_ENGINES (default 2).</summary>
        public int NumEngines { get { int n = ParaformerHip.pf_recognizer_num_engines(_r); ParaformerHip.Check(n < 0 ? n : 0); return n; } }

        /// <summary>Not in the reference: decoding beyond it for every GetResults that follows (off by default).  ctc (SenseVoice
        /// models): the streams' Tokens are the CTC-collapsed ids (repeats merged, blanks dropped, nothing read past the
        /// utterance's own frames), Timestamps one [begin, end] pair in milliseconds per token, Scores the token confidences.
        /// scores alone: Scores holds the log-prob of every position of Tokens.</summary>
        public void SetDecode(bool ctc = false, bool scores = false)
            => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_decode(_r, (ctc ? ParaformerHip.PF_DECODE_CTC : 0) |
                                                                              (scores ? ParaformerHip.PF_DECODE_SCORES : 0)));

        /// <summary>Not in the reference: alternatives for every GetResults that follows (off by default; N = 0 turns them off
        /// again).  Each stream then carries TokenAlternatives, the K (1 .. 8) best (id, log-prob) pairs per token, and —
        /// paraformer models, N &gt; 1 — Alternatives, the exact N-best (&lt;= 64) hypotheses with their scores.  Tokens,
        /// Timestamps, Scores and the result text stay as they are.</summary>
        public void SetNBest(int N, int K = 4) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_nbest(_r, N, K));

        /// <summary>Not in the reference: SenseVoice models only.  A CTC prefix beam search on the device for every GetResults that
        /// follows (off by default; N = 0 turns it off again): each stream's Alternatives holds up to N (&lt;= 64) labelings by
        /// descending Score (the log of the summed alignments), found with beam width W (0 = max(16, N)) over the K (1 .. 8) best
        /// ids per frame.  Tokens, Timestamps, Scores and the result text stay as they are.</summary>
        public void SetCtcBeam(int N, int W = 0, int K = 4) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_ctc_beam(_r, N, W, K));

        /// <summary>Not in the reference: SenseVoice models only (SeACo biases through its own decoder).  Hot-word boosting inside
        /// the beam search of SetCtcBeam (inert without it; 0 turns it off): a labeling earns s per token while it spells a hot word,
        /// keeps it when the word completes and loses it when the match breaks.  The hot words of a GetResults call are the union of
        /// its streams' Hotwords (token ids), else the hot-word file's, tokenised per character as the reference does — set
        /// stream.Hotwords ids where sentencepiece pieces are needed.  Alternatives then come in the biased order, each with Score,
        /// HotwordTokens and LogLikSum; Text and Tokens stay as they are.</summary>
        public void SetHotwordBoost(float s) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_hotword_boost(_r, s));

        /// <summary>Not in the reference: SenseVoice models only.  An ARPA n-gram language model fused into the beam search of
        /// SetCtcBeam (inert without it; null or "" clears it) with weight alpha, per-token bonus beta and flags (1 = add the
        /// end-of-sentence step).  The file is read once against the token table; each engine of the pool uploads it on first use.
        /// Alternatives then come in the fused order, each with Score, LmSum and LogLikSum; Text and Tokens stay as they are.</summary>
        public void SetLm(string? arpaPath, float alpha = 0.5f, float beta = 0f, int flags = 0) =>
            ParaformerHip.Check(ParaformerHip.pf_recognizer_set_lm(_r, arpaPath, alpha, beta, flags));

        /// <summary>Not in the reference: paraformer models only (0 = off, which any model accepts).  The n-best list of
        /// SetNBest(N &gt; 1, K) from a beam search of width max(W, N) over the per-token alternatives on the device (inert until
        /// SetNBest).  Its purpose is SetNBestLm and SetNBestHotwordBoost, whose scores decide which prefixes survive a position.
        /// Alternatives then come in the fused order, each with Score, LogLikSum, LmSum and HotwordTokens; Text, Tokens, Timestamps,
        /// Scores and TokenAlternatives stay as they are.  Not available beside SetVad.</summary>
        public void SetNBestSearch(int W) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_nbest_search(_r, W));

        /// <summary>Not in the reference: paraformer models only.  An ARPA n-gram language model fused into the search of
        /// SetNBestSearch (inert without it; null or "" clears it) with weight alpha, per-token bonus beta and flags.  A paraformer
        /// emits its own end-of-sentence token, which the model already scores: leave flag 1 clear.</summary>
        public void SetNBestLm(string? arpaPath, float alpha = 0.5f, float beta = 0f, int flags = 0) =>
            ParaformerHip.Check(ParaformerHip.pf_recognizer_set_nbest_lm(_r, arpaPath, alpha, beta, flags));

        /// <summary>Not in the reference: paraformer models only.  Hot-word boosting inside the search of SetNBestSearch (inert
        /// without it; 0 turns it off); the hot words are read where SetHotwordBoost reads them.</summary>
        public void SetNBestHotwordBoost(float s) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_nbest_hotword_boost(_r, s));

        /// <summary>Not in the reference: SenseVoice models only.  CTC forced alignment on the device for every GetResults that
        /// follows (off by default): a stream with a target (OfflineStream.SetAlignIds) gets OfflineStream.Alignment, and with
        /// SetCtcBeam every Alternative gets Timestamps of its own and LogLik.  Everything else stays as it is.</summary>
        public void SetAlign(bool on = true) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_align(_r, on ? 1 : 0));

        /// <summary>Not in the reference: long-audio recognition for every GetResults that follows (off by default; null turns it
        /// off again).  Each stream is cut into speech segments on the device, the call's segments are batched by length, forwarded
        /// where they lie and stitched into one result per stream: Text joined by sep, Tokens / Scores concatenated, Timestamps on
        /// the stream's clock; OfflineStream.Segments lists the pieces.  batchMax / frameBudget: 0 = 32 rows / 96000 frames per
        /// batch.  Not available beside SetNBest, SetCtcBeam or SetAlign.  The default thresholds are unvalidated on real speech.</summary>
        public void SetVad(PfVadConfig? cfg, int batchMax = 0, long frameBudget = 0, string sep = "")
        {
            ParaformerHip.Check(ParaformerHip.pf_recognizer_set_vad(_r, cfg == null ? null : new[] { cfg.Value }, batchMax, frameBudget, sep));
        }

        /// <summary>Not in the reference: the FSMN-VAD model score for SetVad's segmentation: a .pfw of kind "fsmnvad", loaded once and
        /// attached to every engine of the pool, present and future; null clears.  Inert until SetVad, and may be set before or after
        /// it; pass DefaultVadModel() to SetVad for the thresholds that go with it (stated, not tuned).</summary>
        public void SetVadModel(string? pfwPath) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_vad_model(_r, pfwPath));

        /// <summary>Not in the reference: punctuation for every GetResults that follows: a .pfw of kind "cttransformer", loaded once and
        /// attached to every engine of the pool; null clears.  Each stream's final Text is punctuated on the device, all streams of a
        /// call in one batch (OfflineStream.Punctuated, PuncIds, Sentences); Text, Tokens and Timestamps stay what they are.  The rules
        /// and dimensions are stated, not validated on a real model.</summary>
        public void SetPuncModel(string? pfwPath) => ParaformerHip.Check(ParaformerHip.pf_recognizer_set_punc_model(_r, pfwPath));

        /// <summary>Not in the reference: speaker labels for every long-audio GetResults that follows (pf_recognizer_set_spk_model): a
        /// .pfw of kind "campplus", loaded once and attached to every engine of the pool; null clears.  cfg: null for the defaults
        /// (DefaultSpeaker()).  Inert until SetVad, before or after it.  OfflineStream.SegmentSpeakers, SpeakerCentroid, SpeakerWindow;
        /// everything else of a result stays what it is.  Nothing of this has been validated on a real model.</summary>
        public void SetSpeakerModel(string? pfwPath, PfSpkConfig? cfg = null)
        {
            PfSpkConfig c = cfg ?? DefaultSpeaker();
            ParaformerHip.Check(ParaformerHip.pf_recognizer_set_spk_model(_r, pfwPath, ref c));
        }

        /// <summary>The stated defaults of the speaker labels (pf_spk_default).</summary>
        public static PfSpkConfig DefaultSpeaker()
        {
            ParaformerHip.Check(ParaformerHip.pf_spk_default(out PfSpkConfig c));
            return c;
        }

        /// <summary>The stated defaults that go with the model score (pf_vad_model_config: floor_pct = -1, abs_level = 9830).</summary>
        public static PfVadConfig DefaultVadModel()
        {
            ParaformerHip.Check(ParaformerHip.pf_vad_model_config(out PfVadConfig c));
            return c;
        }

        /// <summary>The stated defaults of the detector (pf_vad_default).</summary>
        public static PfVadConfig DefaultVad()
        {
            ParaformerHip.Check(ParaformerHip.pf_vad_default(out PfVadConfig c));
            return c;
        }

        public OfflineStream CreateOfflineStream()
        {
            ParaformerHip.Check(ParaformerHip.pf_recognizer_create_stream(_r, out IntPtr s));
            return new OfflineStream(s);
        }

        public OfflineRecognizerResultEntity GetResult(OfflineStream stream) => GetResults(new List<OfflineStream> { stream })[0];

        public List<OfflineRecognizerResultEntity> GetResults(List<OfflineStream> streams)
        {
            var hs = new IntPtr[Math.Max(streams.Count, 1)];
            for (int i = 0; i < streams.Count; i++) hs[i] = streams[i].Handle;
            ParaformerHip.Check(ParaformerHip.pf_recognizer_get_results(_r, hs, streams.Count));
            var res = new List<OfflineRecognizerResultEntity>();
            for (int i = 0; i < streams.Count; i++)
            {
                var e = new OfflineRecognizerResultEntity();
                ParaformerHip.Check(ParaformerHip.pf_result_text(_r, i, out IntPtr txt, out int len16));
                e.Text = Marshal.PtrToStringUTF8(txt);
                e.TextLen = len16;
                ParaformerHip.Check(ParaformerHip.pf_result_num_tokens(_r, i, out int nt));
                for (int j = 0; j < nt; j++)
                {
                    ParaformerHip.Check(ParaformerHip.pf_result_token(_r, i, j, out IntPtr t));
                    e.Tokens.Add(Marshal.PtrToStringUTF8(t) ?? "");
                }
                ParaformerHip.Check(ParaformerHip.pf_result_num_timestamps(_r, i, out int nts));
                for (int j = 0; j < nts; j++)
                {
                    ParaformerHip.Check(ParaformerHip.pf_result_timestamp(_r, i, j, out IntPtr p, out int k));
                    var a = new int[k];
                    if (k > 0) Marshal.Copy(p, a, 0, k);
                    e.Timestamps.Add(a);
                }
                res.Add(e);
            }
            return res;
        }

        public void DisposeOfflineStream(OfflineStream offlineStream) => offlineStream?.Dispose();

        public void Dispose()
        {
            // frees the engine(s) now; later calls answer ObjectDisposedException.  The finaliser is NOT suppressed: it
            // releases the handle shell (pf_recognizer_free), exactly as OfflineStream does above.
            if (_r != IntPtr.Zero) ParaformerHip.pf_recognizer_dispose(_r);
        }
        ~OfflineRecognizer() { if (_r != IntPtr.Zero) { ParaformerHip.pf_recognizer_free(_r); _r = IntPtr.Zero; } }
    }
}
