// OnlineRecognizerHip.cs — drop-in classes with the public signatures of the streaming recogniser
// (AliParaformerAsr/OnlineRecognizer.cs:22,27,32,41,533) and OnlineStream (OnlineStream.cs), backed by the native
// mirror pf_online_* (include/paraformer_hip.h section 7): chunking, feature caches, DynamicMask, the carried-integrator
// CIF and DecodeMulti run behind the C ABI exactly where the reference runs them; only samples go in and text comes out.
// Not compiled in this repository's build image (no .NET toolchain); the same entry points are exercised through the
// Python binding aliparaformerasr_amd/online_recognizer.py by tests/test_gpu_online.py.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using AliParaformerAsr.Model;
using AliParaformerAsr.Native;

namespace AliParaformerAsr.Hip
{
    internal static class OnlineNative
    {
        const string Lib = "paraformer_hip";
        [DllImport(Lib)] internal static extern int pf_online_recognizer_create(string encoderPath, string decoderPath, string configPath,
            string mvnPath, string tokensPath, int threadsNum, int device, out IntPtr recognizer);
        [DllImport(Lib)] internal static extern void pf_online_recognizer_dispose(IntPtr r);
        [DllImport(Lib)] internal static extern void pf_online_recognizer_free(IntPtr r);
        [DllImport(Lib)] internal static extern int pf_online_create_stream(IntPtr r, out IntPtr stream);
        [DllImport(Lib)] internal static extern int pf_online_stream_add_samples(IntPtr s, float[] samples, long n);
        [DllImport(Lib)] internal static extern int pf_online_get_results(IntPtr r, IntPtr[] streams, int nStreams);
        [DllImport(Lib)] internal static extern int pf_online_result_text(IntPtr r, int i, out IntPtr utf8);
        // streaming endpointing and the second pass (paraformer_hip.h "Streaming endpointing and the second pass")
        [DllImport(Lib)] internal static extern int pf_online_recognizer_set_endpoint(IntPtr r, ref PfEndpointConfig cfg);
        [DllImport(Lib)] internal static extern int pf_online_recognizer_set_endpoint(IntPtr r, IntPtr cfgNull);          // IntPtr.Zero: off
        [DllImport(Lib)] internal static extern int pf_online_recognizer_set_endpoint_model(IntPtr r, [MarshalAs(UnmanagedType.LPUTF8Str)] string? pfwPath);
        [DllImport(Lib)] internal static extern int pf_online_recognizer_set_second_pass(IntPtr r, IntPtr offlineRecognizer);
        [DllImport(Lib)] internal static extern int pf_online_stream_input_finished(IntPtr s);
        [DllImport(Lib)] internal static extern int pf_online_stream_num_sentences(IntPtr s, out int n);
        [DllImport(Lib)] internal static extern int pf_online_stream_sentence(IntPtr s, int j, out int beginMs, out int endMs, out int kind,
            out IntPtr firstPassUtf8, out IntPtr textUtf8);
        [DllImport(Lib)] internal static extern int pf_online_stream_sentence_result(IntPtr s, int j, out IntPtr offlineStream);
        [DllImport(Lib)] internal static extern int pf_online_stream_in_speech(IntPtr s, out int inSpeech, out int beginMs);
        [DllImport(Lib)] internal static extern int pf_online_recognizer_set_token_info(IntPtr r, int on);
        [DllImport(Lib)] internal static extern int pf_online_stream_token_info(IntPtr s, out IntPtr toks, out int n);
        [DllImport(Lib)] internal static extern int pf_online_stream_sentence_tokens(IntPtr s, int j, out IntPtr toks, out int n);
        [DllImport(Lib)] internal static extern void pf_online_stream_dispose(IntPtr s);
        [DllImport(Lib)] internal static extern void pf_online_stream_free(IntPtr s);
    }

    public sealed class OnlineStream : IDisposable
    {
        internal IntPtr Handle;
        internal OnlineStream(IntPtr h) { Handle = h; }

        // OnlineStream.AddSamples: appends audio; the library cuts it into 60-frame chunks and keeps the caches
        public void AddSamples(float[] samples)
            => ParaformerHip.Check(OnlineNative.pf_online_stream_add_samples(Handle, samples, samples == null ? 0 : samples.LongLength));

        // no more audio follows: the tail is decoded, the next GetResults flushes the endpoint detector
        public void InputFinished() => ParaformerHip.Check(OnlineNative.pf_online_stream_input_finished(Handle));

        // the sentences the endpoint detector has closed so far
        public int NumSentences
        {
            get { ParaformerHip.Check(OnlineNative.pf_online_stream_num_sentences(Handle, out int n)); return n; }
        }

        // pf_online_token, 24 bytes: id, time_ms, entry, score, flags (flags 1: a token this stream fired; 2: TimeMs is set)
        [StructLayout(LayoutKind.Sequential)]
        public struct OnlineToken { public long Id; public int TimeMs; public int Entry; public float Score; public int Flags; }

        static OnlineToken[] ReadTokens(IntPtr p, int n)
        {
            var t = new OnlineToken[n];
            for (int i = 0; i < n; ++i) t[i] = Marshal.PtrToStructure<OnlineToken>(p + 24 * i);
            return t;
        }

        // OnlineRecognizer.SetTokenInfo: what is known about Tokens[i], index for index.  TimeMs is the start of the 60 ms frame
        // in which the integrator crossed the threshold: not a word boundary, not validated on real speech.
        public OnlineToken[] TokenInfo
        {
            get { ParaformerHip.Check(OnlineNative.pf_online_stream_token_info(Handle, out IntPtr p, out int n)); return ReadTokens(p, n); }
        }

        // the token info sentence j kept from its first pass
        public OnlineToken[] SentenceTokens(int j)
        {
            ParaformerHip.Check(OnlineNative.pf_online_stream_sentence_tokens(Handle, j, out IntPtr p, out int n));
            return ReadTokens(p, n);
        }

        public void Dispose()
        {
            if (Handle == IntPtr.Zero) return;
            OnlineNative.pf_online_stream_dispose(Handle);      // idempotent; later calls answer PF_ERR_DISPOSED
            OnlineNative.pf_online_stream_free(Handle);
            Handle = IntPtr.Zero;
            GC.SuppressFinalize(this);
        }
        ~OnlineStream() { Dispose(); }
    }

    public sealed class OnlineRecognizer : IDisposable
    {
        IntPtr _h;

        // OnlineRecognizer.cs:22 — encoderFilePath names the .pfw container that holds both graphs' tensors
        // (python -m aliparaformerasr_amd.convert); decoderFilePath is accepted and unused; `device` is the extra argument
        public OnlineRecognizer(string encoderFilePath, string decoderFilePath, string configFilePath, string mvnFilePath,
                                string tokensFilePath, int threadsNum = 1, int device = 0)
            => ParaformerHip.Check(OnlineNative.pf_online_recognizer_create(encoderFilePath, decoderFilePath, configFilePath,
                                                                          mvnFilePath, tokensFilePath, threadsNum, device, out _h));

        public OnlineStream CreateOnlineStream()                                                   // :27
        {
            ParaformerHip.Check(OnlineNative.pf_online_create_stream(_h, out IntPtr s));
            return new OnlineStream(s);
        }

        public OnlineRecognizerResultEntity GetResult(OnlineStream stream)                          // :32
            => GetResults(new List<OnlineStream> { stream })[0];

        public List<OnlineRecognizerResultEntity> GetResults(List<OnlineStream> streams)           // :41
        {
            var hs = new IntPtr[streams.Count];
            for (int i = 0; i < hs.Length; i++) hs[i] = streams[i].Handle;
            ParaformerHip.Check(OnlineNative.pf_online_get_results(_h, hs, hs.Length));
            var res = new List<OnlineRecognizerResultEntity>(hs.Length);
            for (int i = 0; i < hs.Length; i++)
            {
                ParaformerHip.Check(OnlineNative.pf_online_result_text(_h, i, out IntPtr p));
                string text = Marshal.PtrToStringUTF8(p) ?? string.Empty;
                res.Add(new OnlineRecognizerResultEntity { Text = text, TextLen = text.Length });
            }
            return res;
        }

        // Endpoint detection for every GetResults that follows (no counterpart in the reference; null: off).  The defaults
        // (pf_endpoint_default) are stated, not tuned: nobody has measured them on real speech.
        public void SetEndpoint(PfEndpointConfig? cfg)
        {
            if (cfg == null) { ParaformerHip.Check(OnlineNative.pf_online_recognizer_set_endpoint(_h, IntPtr.Zero)); return; }
            PfEndpointConfig c = cfg.Value;
            ParaformerHip.Check(OnlineNative.pf_online_recognizer_set_endpoint(_h, ref c));
        }

        // The FSMN-VAD model score as the detector's level (a .pfw of kind "fsmnvad"; null: the energy level).  Inert until
        // SetEndpoint; pass pf_endpoint_model_config's thresholds there (stated, not tuned).
        public void SetEndpointModel(string? pfwPath)
            => ParaformerHip.Check(OnlineNative.pf_online_recognizer_set_endpoint_model(_h, pfwPath));

        // Token times and scores: the chunk step stays on the device and every stream fills OnlineStream.TokenInfo.  Refused once
        // a live stream has decoded a chunk.
        public void SetTokenInfo(bool on = true)
            => ParaformerHip.Check(OnlineNative.pf_online_recognizer_set_token_info(_h, on ? 1 : 0));

        // the offline recognizer's native handle that re-recognises every finished sentence (IntPtr.Zero: none)
        public void SetSecondPass(IntPtr offlineRecognizerHandle)
            => ParaformerHip.Check(OnlineNative.pf_online_recognizer_set_second_pass(_h, offlineRecognizerHandle));

        public void Dispose()                                                                      // :533
        {
            if (_h == IntPtr.Zero) return;
            OnlineNative.pf_online_recognizer_dispose(_h);
            OnlineNative.pf_online_recognizer_free(_h);
            _h = IntPtr.Zero;
            GC.SuppressFinalize(this);
        }
        ~OnlineRecognizer() { Dispose(); }
    }
}
