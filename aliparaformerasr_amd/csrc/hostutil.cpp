// hostutil.cpp — see hostutil.h
#include "hostutil.h"
#include "lm.h"
#include "lm_dev.h"

#include <cerrno>
#include <climits>

#include <cmath>
#include <cstring>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <queue>
#include <sstream>

namespace pf {

bool file_exists(const std::string& path) {
  if (path.empty()) return false;
  std::ifstream f(path, std::ios::binary);
  return f.good();
}

std::string read_text_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f.good()) throw Error(PF_ERR_IO, "cannot open file: " + path);
  std::ostringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

void read_binary_file(const std::string& path, std::vector<char>& out) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f.good()) throw Error(PF_ERR_IO, "cannot open file: " + path);
  const std::streamsize n = f.tellg();
  f.seekg(0);
  out.resize((size_t)n);
  if (n > 0 && !f.read(out.data(), n)) throw Error(PF_ERR_IO, "short read: " + path);
}

std::vector<std::string> split_lines(const std::string& text) {
  // File.ReadAllLines: splits on \n, \r\n, \r; a trailing newline does not create an empty line
  std::vector<std::string> lines;
  size_t i = 0, n = text.size();
  // skip UTF-8 BOM like StreamReader does
  if (n >= 3 && (unsigned char)text[0] == 0xEF && (unsigned char)text[1] == 0xBB && (unsigned char)text[2] == 0xBF) i = 3;
  std::string cur;
  bool any = false;
  for (; i < n; ++i) {
    char c = text[i];
    if (c == '\n' || c == '\r') {
      lines.push_back(cur);
      cur.clear();
      any = false;
      if (c == '\r' && i + 1 < n && text[i + 1] == '\n') ++i;
    } else {
      cur += c;
      any = true;
    }
  }
  if (any) lines.push_back(cur);
  return lines;
}

std::vector<std::string> read_lines(const std::string& path) { return split_lines(read_text_file(path)); }

static std::string trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '\r' || s[a] == '\n')) ++a;
  while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r' || s[b - 1] == '\n')) --b;
  return s.substr(a, b - a);
}

static bool starts_with(const std::string& s, const char* p) { return s.compare(0, std::strlen(p), p) == 0; }

static void parse_bracket_floats(const std::string& line, std::vector<float>& out) {
  const size_t a = line.find('['), b = line.rfind(']');
  if (a == std::string::npos || b == std::string::npos || b <= a)
    throw Error(PF_ERR_FORMAT, "am.mvn: missing [ ] in <LearnRateCoef> line");
  const std::string inner = line.substr(a + 1, b - a - 1);
  out.clear();
  size_t i = 0;
  while (i <= inner.size()) {
    size_t j = inner.find(' ', i);
    if (j == std::string::npos) j = inner.size();
    std::string tok = trim(inner.substr(i, j - i));
    if (!tok.empty()) {
      char* end = nullptr;
      const float v = std::strtof(tok.c_str(), &end);
      if (end == tok.c_str() || *end != '\0') throw Error(PF_ERR_FORMAT, "am.mvn: bad number '" + tok + "'");
      out.push_back(v);
    }
    i = j + 1;
  }
}

void parse_mvn_text(const std::string& text, std::vector<float>& shift, std::vector<float>& scale) {
  shift.clear();
  scale.clear();
  int state = 0;
  for (const std::string& line : split_lines(text)) {
    if (line.empty()) continue;
    if (starts_with(line, "<AddShift>")) { state = 1; continue; }
    if (starts_with(line, "<Rescale>")) { state = 2; continue; }
    if (starts_with(line, "<LearnRateCoef>") && state == 1) { parse_bracket_floats(line, shift); continue; }
    if (starts_with(line, "<LearnRateCoef>") && state == 2) { parse_bracket_floats(line, scale); continue; }
  }
}

// ------------------------------------------------------------------ config ----------------
static std::string unquote(std::string v) {
  v = trim(v);
  if (v.size() >= 2 && ((v.front() == '"' && v.back() == '"') || (v.front() == '\'' && v.back() == '\'')))
    v = v.substr(1, v.size() - 2);
  return v;
}
static bool to_bool(const std::string& v, bool d) {
  std::string s;
  for (char c : v) s += (char)std::tolower((unsigned char)c);
  if (s == "true" || s == "yes" || s == "on" || s == "1") return true;
  if (s == "false" || s == "no" || s == "off" || s == "0") return false;
  return d;
}

// int.Parse-like for the yaml scalars: out-of-range text is a format error (atoi's behaviour there is undefined)
static int yaml_int(const std::string& key, const std::string& v) {
  errno = 0;
  char* end = nullptr;
  const long long x = std::strtoll(v.c_str(), &end, 10);
  if (end == v.c_str() || errno == ERANGE || x < INT32_MIN || x > INT32_MAX)
    throw Error(PF_ERR_FORMAT, "asr.yaml: '" + key + "' is not an integer: '" + v + "'");
  return (int)x;
}

ConfEntity conf_from_yaml(const std::string& text) {
  ConfEntity c;
  std::string section;   // current top-level mapping key
  for (std::string raw : split_lines(text)) {
    // strip comments (outside quotes)
    bool inq = false;
    char qc = 0;
    for (size_t i = 0; i < raw.size(); ++i) {
      if ((raw[i] == '"' || raw[i] == '\'') && (!inq || raw[i] == qc)) { inq = !inq; qc = raw[i]; }
      if (raw[i] == '#' && !inq && (i == 0 || raw[i - 1] == ' ' || raw[i - 1] == '\t')) { raw = raw.substr(0, i); break; }
    }
    if (trim(raw).empty()) continue;
    size_t indent = 0;
    while (indent < raw.size() && raw[indent] == ' ') ++indent;
    const std::string body = trim(raw);
    const size_t colon = body.find(':');
    if (colon == std::string::npos) continue;
    const std::string key = trim(body.substr(0, colon));
    const std::string val = unquote(body.substr(colon + 1));
    if (indent == 0) {
      section = val.empty() ? key : "";
      if (key == "model" && !val.empty()) c.model = val;
      else if (key == "use_itn") c.use_itn = to_bool(val, c.use_itn);
      continue;
    }
    if (section == "frontend_conf") {
      if (key == "fs") c.fs = yaml_int(key, val);
      else if (key == "window") c.window = val;
      else if (key == "n_mels") c.n_mels = yaml_int(key, val);
      else if (key == "frame_length") c.frame_length = yaml_int(key, val);
      else if (key == "frame_shift") c.frame_shift = yaml_int(key, val);
      else if (key == "dither") c.dither = std::strtof(val.c_str(), nullptr);
      else if (key == "lfr_m") c.lfr_m = yaml_int(key, val);
      else if (key == "lfr_n") c.lfr_n = yaml_int(key, val);
      else if (key == "snip_edges") c.snip_edges = to_bool(val, c.snip_edges);
    }
  }
  return c;
}

ConfEntity conf_from_json(const std::string& text) {
  ConfEntity c;
  Json j = JsonParser(text.data(), text.size()).parse();
  c.model = j.str_or("model", c.model);
  c.use_itn = j.bool_or("use_itn", c.use_itn);
  if (const Json* f = j.get("frontend_conf")) {
    c.fs = (int)f->int_or("fs", c.fs, INT32_MIN, INT32_MAX);
    c.window = f->str_or("window", c.window);
    c.n_mels = (int)f->int_or("n_mels", c.n_mels, INT32_MIN, INT32_MAX);
    c.frame_length = (int)f->int_or("frame_length", c.frame_length, INT32_MIN, INT32_MAX);
    c.frame_shift = (int)f->int_or("frame_shift", c.frame_shift, INT32_MIN, INT32_MAX);
    c.dither = (float)f->num_or("dither", c.dither);
    c.lfr_m = (int)f->int_or("lfr_m", c.lfr_m, INT32_MIN, INT32_MAX);
    c.lfr_n = (int)f->int_or("lfr_n", c.lfr_n, INT32_MIN, INT32_MAX);
    c.snip_edges = f->bool_or("snip_edges", c.snip_edges);
  }
  return c;
}

static std::string lower(std::string s) {
  for (char& ch : s) ch = (char)std::tolower((unsigned char)ch);
  return s;
}
static bool ends_with(const std::string& s, const char* suf) {
  const size_t n = std::strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

ConfEntity load_conf(const std::string& path) {
  ConfEntity c;
  if (path.empty()) return c;
  const std::string lp = lower(path);
  if (ends_with(lp, ".json")) {
    if (file_exists(path)) c = conf_from_json(read_text_file(path));
  } else if (ends_with(lp, ".yaml")) {
    if (file_exists(path)) c = conf_from_yaml(read_text_file(path));
  }
  return c;
}

// ------------------------------------------------------------------ UTF-8 -----------------
std::vector<uint32_t> utf8_decode(const std::string& s) {
  std::vector<uint32_t> out;
  size_t i = 0, n = s.size();
  while (i < n) {
    unsigned char c = (unsigned char)s[i];
    uint32_t cp;
    int extra;
    if (c < 0x80) { cp = c; extra = 0; }
    else if ((c >> 5) == 0x6) { cp = c & 0x1F; extra = 1; }
    else if ((c >> 4) == 0xE) { cp = c & 0x0F; extra = 2; }
    else if ((c >> 3) == 0x1E) { cp = c & 0x07; extra = 3; }
    else { cp = 0xFFFD; extra = 0; }
    ++i;
    for (int k = 0; k < extra && i < n; ++k, ++i) cp = (cp << 6) | ((unsigned char)s[i] & 0x3F);
    out.push_back(cp);
  }
  return out;
}

std::string utf8_encode(uint32_t cp) {
  std::string o;
  if (cp < 0x80) o += (char)cp;
  else if (cp < 0x800) { o += (char)(0xC0 | (cp >> 6)); o += (char)(0x80 | (cp & 0x3F)); }
  else if (cp < 0x10000) { o += (char)(0xE0 | (cp >> 12)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
  else { o += (char)(0xF0 | (cp >> 18)); o += (char)(0x80 | ((cp >> 12) & 0x3F)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
  return o;
}

std::string utf8_encode(const std::vector<uint32_t>& cps) {
  std::string o;
  for (uint32_t c : cps) o += utf8_encode(c);
  return o;
}

int utf16_length(const std::string& utf8) {
  int n = 0;
  for (uint32_t cp : utf8_decode(utf8)) n += cp >= 0x10000 ? 2 : 1;
  return n;
}

// ------------------------------------------------------------------ Examples harness -----
bool is_wav_header(const std::string& path) {
  std::vector<char> b;
  if (!file_exists(path)) return false;
  read_binary_file(path, b);
  if (b.size() < 16) return false;
  return std::memcmp(b.data(), "RIFF", 4) == 0 && std::memcmp(b.data() + 8, "WAVE", 4) == 0;
}

static uint32_t rd32(const char* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
static uint16_t rd16(const char* p) { uint16_t v; std::memcpy(&v, p, 2); return v; }

// The RIFF chunk walk (fmt + data) shared by decode_wav_file and pf_host_wav_info.  `b` holds the first `have` bytes of a file of
// `size` bytes: sizes are judged against the file, bytes are read from the prefix; *need_more is set (and nothing else is valid)
// when the walk wants a byte beyond the prefix
static WavInfo wav_info_prefix(const char* b, size_t have, size_t size, const std::string& path, bool* need_more) {
  *need_more = false;
  PF_CHECK(size >= 12 && have >= 12 && std::memcmp(b, "RIFF", 4) == 0 && std::memcmp(b + 8, "WAVE", 4) == 0,
           PF_ERR_FORMAT, "not a RIFF/WAVE file: " + path);
  size_t pos = 12;
  int fmt_tag = 0, bits = 0, block_align = 0;
  WavInfo w;
  bool have_data = false;
  while (pos + 8 <= size) {
    if (pos + 8 > have) { *need_more = true; return w; }
    const uint32_t sz = rd32(b + pos + 4);
    const char* body = b + pos + 8;
    const size_t avail = size - (pos + 8);
    if (std::memcmp(b + pos, "fmt ", 4) == 0 && sz >= 16 && avail >= 16) {
      if (pos + 8 + std::min<size_t>(avail, 26) > have) { *need_more = true; return w; }
      fmt_tag = rd16(body); w.channels = rd16(body + 2); w.sample_rate = (int)rd32(body + 4);
      block_align = rd16(body + 12); bits = rd16(body + 14);
      if (fmt_tag == 0xFFFE && sz >= 26 && avail >= 26) fmt_tag = rd16(body + 24);   // WAVE_FORMAT_EXTENSIBLE sub-format
    } else if (std::memcmp(b + pos, "data", 4) == 0) {
      have_data = true; w.data_offset = pos + 8; w.data_bytes = std::min<size_t>(sz, avail);
      break;
    }
    pos += 8 + (size_t)sz + (sz & 1);
  }
  PF_CHECK(have_data && w.channels > 0 && w.sample_rate > 0 && block_align > 0, PF_ERR_FORMAT, "wav: missing fmt/data chunk: " + path);
  // PCM 8 / 16 / 24 / 32, IEEE float 32 / 64, G.711 A-law (6) and mu-law (7): what NAudio's AudioFileReader turns into float samples
  // for a RIFF/WAVE file (the G.711 forms through a codec that expands them to 16-bit PCM first)
  if (fmt_tag == 1 && bits == 8) w.format = PF_PCM_U8;
  else if (fmt_tag == 1 && bits == 16) w.format = PF_PCM_S16;
  else if (fmt_tag == 1 && bits == 24) w.format = PF_PCM_S24;
  else if (fmt_tag == 1 && bits == 32) w.format = PF_PCM_S32;
  else if (fmt_tag == 3 && bits == 32) w.format = PF_PCM_F32;
  else if (fmt_tag == 3 && bits == 64) w.format = PF_PCM_F64;
  else if (fmt_tag == 6 && bits == 8) w.format = PF_PCM_ALAW;
  else if (fmt_tag == 7 && bits == 8) w.format = PF_PCM_MULAW;
  else throw Error(PF_ERR_UNSUPPORTED, "wav: unsupported sample format");
  w.duration_ms = (double)(w.data_bytes / block_align) * 1000.0 / w.sample_rate;
  return w;
}

WavInfo wav_info(const std::vector<char>& b, const std::string& path) {
  bool more = false;
  return wav_info_prefix(b.data(), b.size(), b.size(), path, &more);
}

// the same from the file, reading the header region only: 64 KiB first, the whole file when a chunk in front of `data` is longer
WavInfo wav_info_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  PF_CHECK((bool)f, PF_ERR_IO, "cannot open file: " + path);
  f.seekg(0, std::ios::end);
  const size_t size = (size_t)std::max<std::streamoff>(f.tellg(), 0);
  std::vector<char> b(std::min<size_t>(size, (size_t)64 << 10));
  f.seekg(0);
  if (!b.empty()) f.read(b.data(), (std::streamsize)b.size());
  PF_CHECK(b.empty() || (size_t)f.gcount() == b.size(), PF_ERR_IO, "cannot read file: " + path);
  bool more = false;
  WavInfo w = wav_info_prefix(b.data(), b.size(), size, path, &more);
  if (!more) return w;
  read_binary_file(path, b);
  return wav_info(b, path);
}

int pcm_bytes_per_value(int format) {
  switch (format) {
    case PF_PCM_U8: case PF_PCM_ALAW: case PF_PCM_MULAW: return 1;
    case PF_PCM_S16: return 2;
    case PF_PCM_S24: return 3;
    case PF_PCM_S32: case PF_PCM_F32: return 4;
    case PF_PCM_F64: return 8;
  }
  throw Error(PF_ERR_INVALID_ARG, "pcm: unknown format " + std::to_string(format));
}

void pcm_decode(const void* data, size_t n, int format, float* out) {
  const int bps = pcm_bytes_per_value(format);
  const unsigned char* d = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) {
    const unsigned char* q = d + i * bps;
    float v;
    if (format == PF_PCM_MULAW) {                        // ITU-T G.711 mu-law: ~byte = sign | exponent (3) | mantissa (4)
      const int u = (~q[0]) & 0xFF;
      const int mag = ((((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84;
      v = (float)((u & 0x80) ? -mag : mag) / 32768.0f;
    } else if (format == PF_PCM_ALAW) {                  // A-law: byte ^ 0x55, sign bit set = positive
      const int a = q[0] ^ 0x55, e = (a >> 4) & 7, m = a & 0x0F;
      const int mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
      v = (float)((a & 0x80) ? mag : -mag) / 32768.0f;
    } else if (format == PF_PCM_F64) { double d; std::memcpy(&d, q, 8); v = (float)d; }
    else if (format == PF_PCM_F32) { std::memcpy(&v, q, 4); }
    else if (format == PF_PCM_S16) { int16_t x; std::memcpy(&x, q, 2); v = x / 32768.0f; }
    else if (format == PF_PCM_S24) { int32_t x = (int32_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)(int8_t)q[2] << 16)); v = x / 8388608.0f; }
    else if (format == PF_PCM_S32) { int32_t x; std::memcpy(&x, q, 4); v = x / 2147483648.0f; }
    else { v = q[0] / 128.0f - 1.0f; }
    out[i] = v;
  }
}

WavData decode_wav_file(const std::string& path) {
  std::vector<char> b;
  read_binary_file(path, b);
  const WavInfo wi = wav_info(b, path);
  WavData w;
  w.sample_rate = wi.sample_rate; w.channels = wi.channels; w.duration_ms = wi.duration_ms;
  const size_t n = wi.data_bytes / pcm_bytes_per_value(wi.format);
  w.samples.resize(n);
  pcm_decode(b.data() + wi.data_offset, n, wi.format, w.samples.data());
  return w;
}

PcmPlan pcm_plan(const pf_pcm_desc& d, int fs, int64_t n_values) {
  PF_CHECK(d.struct_size == (int32_t)sizeof(pf_pcm_desc), PF_ERR_INVALID_ARG, "pf_pcm_desc.struct_size mismatch");
  PF_CHECK(d.channels == 1 || d.channels == 2, PF_ERR_INVALID_ARG, "pcm: only 1 or 2 channels");
  PF_CHECK(d.sample_rate > 0 && fs > 0, PF_ERR_INVALID_ARG, "pcm: sample rates must be positive");
  PF_CHECK(n_values >= 0 && n_values <= INT32_MAX, PF_ERR_INVALID_ARG, "pcm: value count must be in [0, 2^31 - 1]");
  PcmPlan p;
  p.bytes_per_value = pcm_bytes_per_value(d.format);
  p.resample = d.sample_rate != fs;                                     // GetFileSample: resampled (and down-mixed) only then
  p.downmix = d.channels == 2 && (p.resample || (d.flags & PF_PCM_DOWNMIX_ALWAYS));
  p.n_mono = p.downmix ? n_values / 2 : n_values;
  p.ratio = (double)d.sample_rate / fs;
  p.n_out = p.n_mono;
  if (p.resample) {
    const double r = n_values == 0 ? 0.0 : std::nearbyint((double)p.n_mono / p.ratio);   // Math.Round: half to even
    PF_CHECK(r <= (double)INT32_MAX, PF_ERR_INVALID_ARG, "pcm: resampled length exceeds 2^31 - 1");
    p.n_out = std::max((int64_t)r, (int64_t)0);
  }
  return p;
}

std::vector<float> pcm_to_samples(const void* data, int64_t n_values, const pf_pcm_desc& d, int fs) {
  const PcmPlan p = pcm_plan(d, fs, n_values);
  std::vector<float> x((size_t)n_values);
  pcm_decode(data, (size_t)n_values, d.format, x.data());
  if (p.resample) return resample_linear(x, d.sample_rate, fs, d.channels);
  if (p.downmix) {
    std::vector<float> m((size_t)p.n_mono);
    for (size_t i = 0; i < m.size(); ++i) m[i] = (x[2 * i] + x[2 * i + 1]) * 0.5f;
    return m;
  }
  return x;
}

std::vector<float> resample_linear(const std::vector<float>& src, int sr_in, int sr_out, int channels) {
  PF_CHECK(sr_in > 0 && sr_out > 0, PF_ERR_INVALID_ARG, "resample: sample rates must be positive");
  PF_CHECK(channels == 1 || channels == 2, PF_ERR_INVALID_ARG, "resample: only 1 or 2 channels");
  if (src.empty()) return {};
  std::vector<float> mono_buf;
  const std::vector<float>* mono = &src;
  if (channels == 2) {
    mono_buf.resize(src.size() / 2);
    for (size_t i = 0; i < mono_buf.size(); ++i) mono_buf[i] = (src[2 * i] + src[2 * i + 1]) * 0.5f;
    mono = &mono_buf;
  }
  const std::vector<float>& m = *mono;
  const double ratio = (double)sr_in / sr_out;
  const int n_out = (int)std::nearbyint((double)m.size() / ratio);       // Math.Round: half to even
  std::vector<float> out((size_t)std::max(n_out, 0));
  const int last = (int)m.size() - 1;
  for (int i = 0; i < n_out; ++i) {
    const double pos = i * ratio;
    const int idx = (int)pos;
    const double fr = pos - idx;
    if (idx >= last) { out[i] = m[last < 0 ? 0 : last]; continue; }
    out[i] = (float)((1 - fr) * m[idx] + fr * m[idx + 1]);
  }
  return out;
}

std::vector<float> get_file_sample(const std::string& path, double* duration_ms) {
  if (!file_exists(path)) return std::vector<float>(1, 0.f);
  WavData w = decode_wav_file(path);
  if (duration_ms) *duration_ms = w.duration_ms;
  if (w.sample_rate != 16000) return resample_linear(w.samples, w.sample_rate, 16000, w.channels);
  return w.samples;
}

// ------------------------------------------------------------------ n-best ---------------
namespace {
struct NbNode {
  double score;
  std::vector<uint8_t> r;     // ranks (K <= PF_TOPK_MAX)
  int last;                   // the position the last step raised (children raise positions >= last)
};
// true when a comes AFTER b in the list (std::priority_queue keeps the "largest")
struct NbAfter {
  bool operator()(const NbNode& a, const NbNode& b) const {
    if (a.score != b.score) return a.score < b.score;
    return std::lexicographical_compare(b.r.begin(), b.r.end(), a.r.begin(), a.r.end());
  }
};
double nb_score(const float* val, int L, int K, const std::vector<uint8_t>& r) {
  double s = 0.0;
  for (int l = 0; l < L; ++l) s += (double)val[(size_t)l * K + r[(size_t)l]];
  return s;
}
}  // namespace

int host_nbest(const float* val, const int32_t* n, int L, int K, int n_free, int N, int32_t* out_ranks, double* out_scores) {
  if (!val || !n || !out_ranks || !out_scores) throw Error(PF_ERR_INVALID_ARG, "nbest: null argument");
  if (L < 1 || K < 1 || K > PF_TOPK_MAX || N < 1 || N > PF_NBEST_MAX || n_free < 0 || n_free > L)
    throw Error(PF_ERR_INVALID_ARG, "nbest: bad L / K / N / n_free");
  for (int l = 0; l < L; ++l) {
    if (n[l] < 0 || n[l] > K) throw Error(PF_ERR_INVALID_ARG, "nbest: n[l] outside 0 .. K");
    if (n[l] == 0) return 0;                             // a position with no ranked entry: no rank vector exists
    for (int k = 0; k < n[l]; ++k) {
      const float v = val[(size_t)l * K + k];
      if (v != v || v == INFINITY) throw Error(PF_ERR_INVALID_ARG, "nbest: NaN or +inf among the ranked values");
    }
  }
  std::priority_queue<NbNode, std::vector<NbNode>, NbAfter> heap;
  NbNode root;
  root.r.assign((size_t)L, 0);
  root.score = nb_score(val, L, K, root.r);
  root.last = 0;
  heap.push(std::move(root));
  int got = 0;
  while (got < N && !heap.empty()) {
    NbNode cur = heap.top();
    heap.pop();
    for (int l = 0; l < L; ++l) out_ranks[(size_t)got * L + l] = cur.r[(size_t)l];
    out_scores[got] = cur.score;
    ++got;
    if (got == N) break;
    for (int l = cur.last; l < n_free; ++l) {
      if (cur.r[(size_t)l] + 1 >= n[l]) continue;
      NbNode ch;
      ch.r = cur.r;
      ++ch.r[(size_t)l];
      ch.last = l;
      ch.score = nb_score(val, L, K, ch.r);              // from scratch: the sum's rounding is that of the definition
      heap.push(std::move(ch));
    }
  }
  return got;
}

// ------------------------------------------------------------------ CTC prefix beam search ---------------
namespace {
const double kNegInf = -INFINITY;
inline double beam_lse(double a, double b) {
  if (a == kNegInf) return b;
  if (b == kNegInf) return a;
  const double m = a > b ? a : b;
  return m + std::log1p(std::exp(-std::fabs(a - b)));
}
inline uint64_t beam_hash(uint64_t h, int c) {
  h = (h ^ ((uint64_t)(uint32_t)c + 0x9E3779B97F4A7C15ull)) * 0x100000001B3ull;
  return h ^ (h >> 29);
}
struct BeamEntry {
  double pb, pnb;
  uint64_t hash;
  int node, par, tok, len;
  int st, m;                 // hot words: automaton state and matched tokens of the prefix (0 / 0 without a set)
  int ls;                    // language model: its state and g of the prefix (0 / 0 without a model)
  double g;
};
struct BeamCand {
  double tot, key, pb, pnb;  // key = tot + bias(prefix) + g(prefix): what select orders by (tot itself without a set or a model)
  int idx, st, m;
  int ls;
  double g;
};

// the search of the definition; g == nullptr: the unbiased one (tests/ctcbeam_ref.py), else tests/ctcbeam_bias_ref.py; lm: the
// fused one (tests/ctcbeam_lm_ref.py), whose step is lm_dev.h's, the text the kernel runs
int ctc_beam_impl(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int T, int K,
                  int blank, int W, int N, const HotwordGraph* g, double boost, int64_t* out_ids, int32_t* out_len, double* out_score,
                  int32_t* out_matched, double* out_loglik, int cap, const LmImage* lm = nullptr, double alpha = 0.0, double beta = 0.0,
                  int lm_flags = 0, double* out_lm = nullptr) {
  if (!out_ids || !out_len || !out_score || (T > 0 && (!blank_lp || !ids || !val || !n)))
    throw Error(PF_ERR_INVALID_ARG, "ctc_beam: null argument");
  if (T < 0 || K < 1 || K > PF_TOPK_MAX || N < 1 || N > W || W > PF_NBEST_MAX || cap < 0 || blank_stride < 1)
    throw Error(PF_ERR_INVALID_ARG, "ctc_beam: bad T / K / W / N / cap");
  for (int h = 0; h < N; ++h) {
    out_len[h] = 0; out_score[h] = kNegInf;
    if (out_matched) out_matched[h] = 0;
    if (out_loglik) out_loglik[h] = kNegInf;
    if (out_lm) out_lm[h] = 0.0;
  }
  LmView lv{};
  if (lm) lv = lm_view(lm->words.data());
  std::fill(out_ids, out_ids + (size_t)N * cap, (int64_t)-1);
  for (int t = 0; t < T; ++t) {
    if (n[t] < 0 || n[t] > K) throw Error(PF_ERR_INVALID_ARG, "ctc_beam: n[t] outside 0 .. K");
    const float lb = blank_lp[(size_t)t * blank_stride];
    if (n[t] == 0 || lb != lb) return 0;
  }
  // node 0 is the empty prefix; a chain of (parent, token) spells a prefix backwards
  std::vector<int> npar(1, -1), ntok(1, -1);
  auto same_prefix = [&](int a, int b) {           // equally long by the caller's filter
    while (a != b) {
      if (a <= 0 || b <= 0) return false;
      if (ntok[(size_t)a] != ntok[(size_t)b]) return false;
      a = npar[(size_t)a];
      b = npar[(size_t)b];
    }
    return true;
  };
  const int Vg = g ? (int)g->tok_col.size() : 0;
  std::vector<BeamEntry> beam(1, BeamEntry{0.0, kNegInf, 0x243F6A8885A308D3ull, 0, -1, -1, 0, 0, 0, lv.start, 0.0}), next;
  std::vector<BeamCand> cand;
  std::vector<double> merged;
  const int K1 = K + 1;
  for (int t = 0; t < T; ++t) {
    const int64_t* id = ids + (size_t)t * K;
    const float* lp = val + (size_t)t * K;
    const int nt = n[t];
    const double lb = (double)blank_lp[(size_t)t * blank_stride];
    const int nbeam = (int)beam.size();
    cand.assign((size_t)nbeam * K1, BeamCand{kNegInf, kNegInf, kNegInf, kNegInf, 0, 0, 0, 0, 0.0});
    merged.assign((size_t)nbeam, kNegInf);
    for (int i = 0; i < nbeam; ++i) {
      const BeamEntry& p = beam[(size_t)i];
      const double tot = beam_lse(p.pb, p.pnb);
      BeamCand& st = cand[(size_t)i * K1];
      st.pb = tot + lb;
      st.st = p.st; st.m = p.m;
      st.ls = p.ls; st.g = p.g;
      for (int r = 0; r < nt; ++r) {
        const int c = (int)id[r];
        if (c == blank || c < 0) continue;
        if (p.len > 0 && c == p.tok) st.pnb = p.pnb + (double)lp[r];
        const double base = (p.len > 0 && c == p.tok) ? p.pb : tot;
        if (base == kNegInf) continue;
        const double value = base + (double)lp[r];
        const uint64_t h = beam_hash(p.hash, c);
        int hit = -1;
        for (int q = 0; q < nbeam; ++q) {
          const BeamEntry& e = beam[(size_t)q];
          if (e.len == p.len + 1 && e.tok == c && e.hash == h && same_prefix(e.par, p.node)) hit = q;
        }
        if (hit >= 0) { merged[(size_t)hit] = value; continue; }   // at most one extension meets one entry
        BeamCand& x = cand[(size_t)i * K1 + 1 + r];
        x.pnb = value;
        if (g) {
          const int col = c < Vg ? g->tok_col[(size_t)c] : -1;
          const int e = col >= 0 ? g->table[(size_t)p.st * g->A + col] : 0;
          x.st = e & 0xFFFF;
          x.m = p.m + ((e >> 16) & 0xFF);
        }
        if (lm) {
          x.g = p.g;
          x.ls = lm_step(lv, p.ls, c, alpha, beta, true, x.g);
        }
      }
    }
    std::vector<int> live;
    for (int j = 0; j < nbeam * K1; ++j) {
      BeamCand& c = cand[(size_t)j];
      c.idx = j;
      if (j % K1 == 0) c.pnb = beam_lse(c.pnb, merged[(size_t)(j / K1)]);
      c.tot = beam_lse(c.pb, c.pnb);
      c.key = g ? c.tot + boost * (double)(c.m + g->depth[(size_t)c.st]) : c.tot;
      if (lm) c.key = c.key + c.g;
      if (c.tot > kNegInf) live.push_back(j);
    }
    std::sort(live.begin(), live.end(), [&](int a, int b) {
      const double x = cand[(size_t)a].key, y = cand[(size_t)b].key;
      return x != y ? x > y : a < b;
    });
    if ((int)live.size() > W) live.resize((size_t)W);
    next.clear();
    for (int j : live) {
      const BeamCand& c = cand[(size_t)j];
      const BeamEntry& p = beam[(size_t)(j / K1)];
      if (j % K1 == 0) {
        next.push_back(BeamEntry{c.pb, c.pnb, p.hash, p.node, p.par, p.tok, p.len, c.st, c.m, c.ls, c.g});
      } else {
        const int tok = (int)id[j % K1 - 1];
        npar.push_back(p.node);
        ntok.push_back(tok);
        next.push_back(BeamEntry{c.pb, c.pnb, beam_hash(p.hash, tok), (int)npar.size() - 1, p.node, tok, p.len + 1, c.st, c.m, c.ls, c.g});
      }
    }
    beam.swap(next);
  }
  // finish: the pending part of the bias is revoked, the completed part stays; (score, beam rank) orders the output
  const int nb = (int)beam.size();
  std::vector<double> ll((size_t)nb), score((size_t)nb);
  std::vector<int> order((size_t)nb);
  for (int h = 0; h < nb; ++h) {
    ll[(size_t)h] = beam_lse(beam[(size_t)h].pb, beam[(size_t)h].pnb);
    score[(size_t)h] = g ? ll[(size_t)h] + boost * (double)beam[(size_t)h].m : ll[(size_t)h];
    if (lm) {                                        // g_final: the end-of-sentence step where asked for
      BeamEntry& e = beam[(size_t)h];
      if ((lm_flags & PF_LM_EOS) && lv.eos >= 0) lm_step(lv, e.ls, lv.eos, alpha, beta, false, e.g);
      score[(size_t)h] = score[(size_t)h] + e.g;
    }
    order[(size_t)h] = h;
  }
  if (g || lm)
    std::sort(order.begin(), order.end(), [&](int a, int b) {
      return score[(size_t)a] != score[(size_t)b] ? score[(size_t)a] > score[(size_t)b] : a < b;
    });
  const int nh = std::min(N, nb);
  for (int h = 0; h < nh; ++h)
    if (beam[(size_t)order[(size_t)h]].len > cap)
      throw Error(PF_ERR_CAPACITY, "ctc_beam: a hypothesis of " + std::to_string(beam[(size_t)order[(size_t)h]].len) + " tokens > cap");
  for (int h = 0; h < nh; ++h) {
    const int src = order[(size_t)h];
    const BeamEntry& e = beam[(size_t)src];
    int node = e.node;
    for (int p = e.len - 1; p >= 0; --p) { out_ids[(size_t)h * cap + p] = ntok[(size_t)node]; node = npar[(size_t)node]; }
    out_len[h] = e.len;
    out_score[h] = score[(size_t)src];
    if (out_matched) out_matched[h] = e.m;
    if (out_loglik) out_loglik[h] = ll[(size_t)src];
    if (out_lm) out_lm[h] = e.g;
  }
  return nh;
}
}  // namespace

int host_ctc_beam(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int T, int K,
                  int blank, int W, int N, int64_t* out_ids, int32_t* out_len, double* out_score, int cap) {
  return ctc_beam_impl(blank_lp, blank_stride, ids, val, n, T, K, blank, W, N, nullptr, 0.0, out_ids, out_len, out_score, nullptr,
                       nullptr, cap);
}

// ------------------------------------------------------------------ hot words: context graph ---------------
void build_hotword_graph(const int32_t* ids, const int32_t* lens, int n, int V, HotwordGraph& g) {
  if (n < 0 || V < 1 || (n > 0 && !lens)) throw Error(PF_ERR_INVALID_ARG, "hotword_graph: bad n / V / lens");
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (lens[i] < 0) throw Error(PF_ERR_INVALID_ARG, "hotword_graph: negative hot-word length");
    total += (size_t)lens[i];
  }
  if (total > 0 && !ids) throw Error(PF_ERR_INVALID_ARG, "hotword_graph: null ids");
  for (size_t x = 0; x < total; ++x)
    if (ids[x] <= 0 || ids[x] >= V) throw Error(PF_ERR_INVALID_ARG, "hotword_graph: an id outside [1, V)");
  for (int i = 0; i < n; ++i)
    if (lens[i] > PF_HOTWORD_LEN_MAX)
      throw Error(PF_ERR_CAPACITY, "hotword_graph: a hot word of " + std::to_string(lens[i]) + " ids > PF_HOTWORD_LEN_MAX");
  g = HotwordGraph();
  g.tok_col.assign((size_t)V, -1);
  std::vector<int32_t> toks(ids, ids + total);
  std::sort(toks.begin(), toks.end());
  toks.erase(std::unique(toks.begin(), toks.end()), toks.end());
  const int A = (int)toks.size();
  for (int a = 0; a < A; ++a) g.tok_col[(size_t)toks[(size_t)a]] = a;
  // the trie: children as (node, column) -> node; is_end marks a node that spells a whole hot word
  std::map<std::pair<int, int>, int> child;
  std::vector<int> depth(1, 0), parent(1, -1), pcol(1, -1);
  std::vector<char> is_end(1, 0);
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    int u = 0;
    for (int p = 0; p < lens[i]; ++p) {
      const int col = g.tok_col[(size_t)ids[off + p]];
      auto it = child.find({u, col});
      if (it == child.end()) {
        if ((int)depth.size() >= PF_HOTWORD_STATES_MAX)
          throw Error(PF_ERR_CAPACITY, "hotword_graph: more than PF_HOTWORD_STATES_MAX states");
        const int v = (int)depth.size();
        child[{u, col}] = v;
        depth.push_back(depth[(size_t)u] + 1);
        parent.push_back(u);
        pcol.push_back(col);
        is_end.push_back(0);
        u = v;
      } else {
        u = it->second;
      }
    }
    if (lens[i] > 0) is_end[(size_t)u] = 1;
    off += (size_t)lens[i];
  }
  const int S = (int)depth.size();
  if ((size_t)S * (size_t)A * 4 > (size_t)PF_HOTWORD_TABLE_BYTES_MAX)
    throw Error(PF_ERR_CAPACITY, "hotword_graph: a table of " + std::to_string(S) + " x " + std::to_string(A) + " entries > PF_HOTWORD_TABLE_BYTES_MAX");
  g.S = S;
  g.A = A;
  g.depth.assign(depth.begin(), depth.end());
  // the full Aho-Corasick transition delta(u, a) = the longest suffix of path(u) + a that is a trie path, breadth first
  // (nodes were numbered along the words, not by depth, so the order is made here); endlen(v): the longest hot word that
  // is a suffix of path(v), i.e. that ends v or a node on v's failure chain
  std::vector<int32_t> delta((size_t)S * A, 0);
  std::vector<int> fail((size_t)S, 0), endlen((size_t)S, 0), bfs;
  bfs.reserve((size_t)S);
  bfs.push_back(0);
  for (auto& kv : child)
    if (kv.first.first == 0) delta[(size_t)kv.first.second] = kv.second;
  std::vector<std::vector<std::pair<int, int>>> kids((size_t)S);
  for (auto& kv : child) kids[(size_t)kv.first.first].push_back({kv.first.second, kv.second});
  for (size_t head = 0; head < bfs.size(); ++head) {
    const int u = bfs[head];
    if (u != 0) {
      const int f = parent[(size_t)u] == 0 ? 0 : delta[(size_t)fail[(size_t)parent[(size_t)u]] * A + pcol[(size_t)u]];
      fail[(size_t)u] = f;
      endlen[(size_t)u] = is_end[(size_t)u] ? depth[(size_t)u] : endlen[(size_t)f];
      for (int a = 0; a < A; ++a) delta[(size_t)u * A + a] = delta[(size_t)f * A + a];
      for (auto& k : kids[(size_t)u]) delta[(size_t)u * A + k.first] = k.second;
    }
    for (auto& k : kids[(size_t)u]) bfs.push_back(k.second);
  }
  g.table.assign((size_t)S * A, 0);
  for (size_t x = 0; x < (size_t)S * A; ++x) {
    const int v = delta[x];
    g.table[x] = endlen[(size_t)v] > 0 ? (endlen[(size_t)v] << 16) : (v | (depth[(size_t)v] << 24));
  }
}

// one past the largest id of a set given without a vocabulary size (ids below 1 are left to the builder's refusal)
int hotword_vocab_bound(const int32_t* ids, const int32_t* lens, int n) {
  int64_t total = 0;
  for (int i = 0; i < n && lens; ++i) total += std::max(lens[i], 0);
  int mx = 0;
  for (int64_t x = 0; x < total && ids; ++x) mx = std::max(mx, ids[x]);
  if (mx >= (1 << 24)) throw Error(PF_ERR_INVALID_ARG, "ctc_beam_hot: a hot-word id outside [1, 2^24)");
  return mx + 1;
}

int host_ctc_beam_hot(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int T, int K,
                      int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost, int64_t* out_ids,
                      int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap) {
  if (!out_matched || !out_loglik) throw Error(PF_ERR_INVALID_ARG, "ctc_beam_hot: null argument");
  if (!(boost >= 0.f) || std::isinf(boost)) throw Error(PF_ERR_INVALID_ARG, "ctc_beam_hot: the boost is finite and >= 0");
  HotwordGraph g;
  build_hotword_graph(hw_ids, hw_lens, n_hw, hotword_vocab_bound(hw_ids, hw_lens, n_hw), g);
  const bool on = boost > 0.f && !g.empty();
  const int nh = ctc_beam_impl(blank_lp, blank_stride, ids, val, n, T, K, blank, W, N, on ? &g : nullptr, (double)boost, out_ids, out_len,
                               out_score, out_matched, out_loglik, cap);
  return nh;
}

int host_ctc_beam_lm(const float* blank_lp, int64_t blank_stride, const int64_t* ids, const float* val, const int32_t* n, int T, int K,
                     int blank, int W, int N, const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost, int64_t* out_ids,
                     int32_t* out_len, double* out_score, int32_t* out_matched, double* out_loglik, int cap, const LmImage& lm, float alpha,
                     float beta, int lm_flags, double* out_lm) {
  if (!out_matched || !out_loglik || !out_lm) throw Error(PF_ERR_INVALID_ARG, "ctc_beam_lm: null argument");
  if (!(boost >= 0.f) || std::isinf(boost)) throw Error(PF_ERR_INVALID_ARG, "ctc_beam_hot: the boost is finite and >= 0");
  if (!(alpha >= 0.f) || std::isinf(alpha) || !std::isfinite(beta) || (lm_flags & ~PF_LM_EOS))
    throw Error(PF_ERR_INVALID_ARG, "lm: alpha is finite and >= 0, beta finite, flags known");
  HotwordGraph g;
  build_hotword_graph(hw_ids, hw_lens, n_hw, hotword_vocab_bound(hw_ids, hw_lens, n_hw), g);
  const bool on = boost > 0.f && !g.empty();
  return ctc_beam_impl(blank_lp, blank_stride, ids, val, n, T, K, blank, W, N, on ? &g : nullptr, (double)boost, out_ids, out_len, out_score,
                       out_matched, out_loglik, cap, &lm, (double)alpha, (double)beta, lm_flags, out_lm);
}

// ------------------------------------------------------------------ n-best search (paraformer) ---------------
int host_nbest_search(const int64_t* ids, const float* val, const int32_t* n, int L, int K, int token_num, int W, int N,
                      const int32_t* hw_ids, const int32_t* hw_lens, int n_hw, float boost, const LmImage* lm, float alpha, float beta,
                      int lm_flags, int32_t* out_ranks, double* out_score, double* out_loglik, double* out_lm, int32_t* out_matched) {
  if (L < 0 || K < 1 || K > PF_TOPK_MAX || N < 1 || N > W || W > PF_NBEST_MAX)
    throw Error(PF_ERR_INVALID_ARG, "nbest_search: bad L / K / W / N");
  if (L > 0 && (!ids || !val || !n || !out_ranks)) throw Error(PF_ERR_INVALID_ARG, "nbest_search: null argument");
  if (!(boost >= 0.f) || std::isinf(boost)) throw Error(PF_ERR_INVALID_ARG, "nbest_search: the boost is finite and >= 0");
  // (stated here as in host_ctc_beam_lm: this file links without lm.cpp)
  if (lm && (!(alpha >= 0.f) || std::isinf(alpha) || !std::isfinite(beta) || (lm_flags & ~PF_LM_EOS)))
    throw Error(PF_ERR_INVALID_ARG, "lm: alpha is finite and >= 0, beta finite, flags known");
  HotwordGraph graph;
  if (n_hw != 0) build_hotword_graph(hw_ids, hw_lens, n_hw, hotword_vocab_bound(hw_ids, hw_lens, n_hw), graph);
  const HotwordGraph* g = boost > 0.f && !graph.empty() ? &graph : nullptr;
  const double s = (double)boost, al = (double)alpha, be = (double)beta;
  for (int h = 0; h < N; ++h) {
    if (out_score) out_score[h] = kNegInf;
    if (out_loglik) out_loglik[h] = kNegInf;
    if (out_lm) out_lm[h] = 0.0;
    if (out_matched) out_matched[h] = 0;
  }
  if (L > 0) std::fill(out_ranks, out_ranks + (size_t)N * L, -1);
  bool ok = L > 0;
  for (int l = 0; l < L; ++l) {
    if (n[l] < 0 || n[l] > K) throw Error(PF_ERR_INVALID_ARG, "nbest_search: n[l] outside 0 .. K");
    if (n[l] == 0) ok = false;
    for (int r = 0; r < n[l]; ++r) {
      const float v = val[(size_t)l * K + r];
      if (v != v || v == INFINITY) ok = false;
    }
  }
  if (!ok) return 0;
  const int n_free = std::min(L, std::max(token_num, 0));
  LmView lv{};
  if (lm) lv = lm_view(lm->words.data());
  const int Vg = g ? (int)g->tok_col.size() : 0;
  struct Entry { double a, g; int ls, st, m; };
  struct Cand { double key; Entry e; int parent, r; };
  std::vector<Entry> beam(1, Entry{0.0, 0.0, lv.start, 0, 0}), next;
  std::vector<Cand> cand;
  std::vector<int> order;
  std::vector<int32_t> bp((size_t)n_free * W, 0);    // (parent slot << 8) | r per (l, slot), as the kernel keeps them
  for (int l = 0; l < n_free; ++l) {
    cand.clear();
    for (int i = 0; i < (int)beam.size(); ++i)
      for (int r = 0; r < n[l]; ++r) {
        const Entry& p = beam[(size_t)i];
        const int c = (int)ids[(size_t)l * K + r];
        Cand x{0.0, p, i, r};
        x.e.a = p.a + (double)val[(size_t)l * K + r];
        x.key = x.e.a;
        if (g) {
          const int col = c >= 0 && c < Vg ? g->tok_col[(size_t)c] : -1;
          const int e = col >= 0 ? g->table[(size_t)p.st * g->A + col] : 0;
          x.e.st = e & 0xFFFF;
          x.e.m = p.m + ((e >> 16) & 0xFF);
          x.key = x.key + s * (double)(x.e.m + g->depth[(size_t)x.e.st]);
        }
        if (lm) {
          x.e.ls = lm_step(lv, p.ls, c, al, be, true, x.e.g);
          x.key = x.key + x.e.g;
        }
        cand.push_back(x);
      }
    order.resize(cand.size());
    for (size_t j = 0; j < cand.size(); ++j) order[j] = (int)j;
    std::sort(order.begin(), order.end(), [&](int x, int y) {   // (the candidate index i * K + r orders as the place in `cand` does)
      return cand[(size_t)x].key != cand[(size_t)y].key ? cand[(size_t)x].key > cand[(size_t)y].key : x < y;
    });
    if ((int)order.size() > W) order.resize((size_t)W);
    next.clear();
    for (size_t slot = 0; slot < order.size(); ++slot) {
      const Cand& x = cand[(size_t)order[slot]];
      next.push_back(x.e);
      bp[(size_t)l * W + slot] = (x.parent << 8) | x.r;
    }
    beam.swap(next);
  }
  const int nb = (int)beam.size();
  std::vector<double> score((size_t)nb);
  order.resize((size_t)nb);
  for (int h = 0; h < nb; ++h) {
    Entry& e = beam[(size_t)h];
    for (int l = n_free; l < L; ++l) e.a = e.a + (double)val[(size_t)l * K];
    double sc = e.a;
    if (g) sc = sc + s * (double)e.m;
    if (lm) {
      if ((lm_flags & PF_LM_EOS) && lv.eos >= 0) lm_step(lv, e.ls, lv.eos, al, be, false, e.g);
      sc = sc + e.g;
    }
    score[(size_t)h] = sc;
    order[(size_t)h] = h;
  }
  std::sort(order.begin(), order.end(), [&](int x, int y) {
    return score[(size_t)x] != score[(size_t)y] ? score[(size_t)x] > score[(size_t)y] : x < y;
  });
  const int nh = std::min(N, nb);
  for (int h = 0; h < nh; ++h) {
    int slot = order[(size_t)h];
    const Entry& e = beam[(size_t)slot];
    if (out_score) out_score[h] = score[(size_t)slot];
    if (out_loglik) out_loglik[h] = e.a;
    if (out_lm) out_lm[h] = e.g;
    if (out_matched) out_matched[h] = e.m;
    int32_t* rk = out_ranks + (size_t)h * L;
    for (int l = n_free; l < L; ++l) rk[l] = 0;
    for (int l = n_free - 1; l >= 0; --l) {
      const int v = bp[(size_t)l * W + slot];
      rk[l] = v & 0xFF;
      slot = v >> 8;
    }
  }
  return nh;
}

// ------------------------------------------------------------------ CTC forced alignment ---------------
int host_ctc_align(const float* lp, int64_t ld, int T, int V, const int64_t* y, int U, float* path_score, double* loglik,
                   int32_t* first, int32_t* last, float* tok_score) {
  if (!path_score || !loglik || (U > 0 && (!y || !first || !last || !tok_score)) || (T > 0 && !lp))
    throw Error(PF_ERR_INVALID_ARG, "ctc_align: null argument");
  if (T < 0 || U < 0 || V < 1 || ld < V) throw Error(PF_ERR_INVALID_ARG, "ctc_align: bad T / U / V / ld");
  if (U > PF_ALIGN_MAX_TOKENS) throw Error(PF_ERR_CAPACITY, "ctc_align: a target of " + std::to_string(U) + " tokens > PF_ALIGN_MAX_TOKENS");
  for (int u = 0; u < U; ++u)
    if (y[u] < 1 || y[u] >= V) throw Error(PF_ERR_INVALID_ARG, "ctc_align: a target id outside [1, V)");
  const float kNegF = -INFINITY;
  for (int u = 0; u < U; ++u) { first[u] = -1; last[u] = -1; tok_score[u] = 0.f; }
  if (T == 0) {
    *path_score = U == 0 ? 0.f : kNegF;
    *loglik = U == 0 ? 0.0 : kNegInf;
    return U == 0;
  }
  const int S = 2 * U + 1, nW = (S + 15) / 16;
  auto lab = [&](int s) { return (s & 1) ? (int)y[s >> 1] : 0; };
  std::vector<float> a((size_t)S, kNegF), na((size_t)S);
  std::vector<double> d((size_t)S, kNegInf), nd((size_t)S);
  std::vector<uint32_t> bp((size_t)T * nW, 0u);         // 2 bits per cell, 16 states per word, as the kernel packs them
  a[0] = lp[0]; d[0] = (double)lp[0];
  if (S > 1) { a[1] = lp[lab(1)]; d[1] = (double)a[1]; }
  for (int t = 1; t < T; ++t) {
    const float* row = lp + (size_t)t * ld;
    for (int s = 0; s < S; ++s) {
      const bool skip = (s & 1) && s >= 3 && lab(s) != lab(s - 2);
      float best = a[(size_t)s];
      uint32_t m = 0;
      if (s >= 1 && a[(size_t)s - 1] > best) { best = a[(size_t)s - 1]; m = 1; }
      if (skip && a[(size_t)s - 2] > best) { best = a[(size_t)s - 2]; m = 2; }
      const float v = row[lab(s)];
      na[(size_t)s] = best + v;
      bp[(size_t)t * nW + (s >> 4)] |= m << (2 * (s & 15));
      double acc = d[(size_t)s];
      if (s >= 1) acc = beam_lse(acc, d[(size_t)s - 1]);
      if (skip) acc = beam_lse(acc, d[(size_t)s - 2]);
      nd[(size_t)s] = acc + (double)v;
    }
    a.swap(na);
    d.swap(nd);
  }
  int s = S - 1;
  if (S > 1 && a[(size_t)S - 2] > a[(size_t)S - 1]) s = S - 2;
  *path_score = a[(size_t)s];
  *loglik = S > 1 ? beam_lse(d[(size_t)S - 1], d[(size_t)S - 2]) : d[0];
  if (!(*path_score > kNegF)) return 0;
  for (int t = T - 1; t >= 0; --t) {
    if (s & 1) {
      const int u = s >> 1;
      const float v = lp[(size_t)t * ld + y[u]];
      if (last[u] < 0) { last[u] = t; tok_score[u] = v; }
      else tok_score[u] = fmaxf(tok_score[u], v);
      first[u] = t;
    }
    s -= (int)((bp[(size_t)t * nW + (s >> 4)] >> (2 * (s & 15))) & 3u);
  }
  return 1;
}


// ---- voice-activity segmentation (paraformer_hip.h "Voice-activity segmentation"; tests/vad_ref.py) --------------------------
pf_vad_config vad_default() {
  pf_vad_config c{};
  c.struct_size = (int32_t)sizeof(pf_vad_config);
  c.floor_pct = 10; c.margin_q = 96; c.abs_level = INT32_MIN;
  c.window = 20; c.on_count = 15; c.off_count = 15;
  c.pad_begin = 30; c.pad_end = 5;
  c.min_speech = 50; c.max_len = 3000; c.split_search = 500;
  return c;
}

pf_vad_config vad_check(const pf_vad_config* cfg, int lfr_n) {
  if (!cfg) return vad_default();
  const pf_vad_config c = *cfg;
  PF_CHECK(c.struct_size == (int32_t)sizeof(pf_vad_config), PF_ERR_INVALID_ARG, "pf_vad_config.struct_size mismatch");
  PF_CHECK(c.floor_pct >= -1 && c.floor_pct <= 100, PF_ERR_INVALID_ARG, "vad: floor_pct outside -1 .. 100");
  PF_CHECK(c.window >= 1 && c.window <= 256, PF_ERR_INVALID_ARG, "vad: window outside 1 .. 256");
  PF_CHECK(c.on_count >= 1 && c.on_count <= c.window && c.off_count >= 1 && c.off_count <= c.window, PF_ERR_INVALID_ARG,
           "vad: on_count / off_count outside 1 .. window");
  PF_CHECK(c.on_count + c.off_count > c.window, PF_ERR_INVALID_ARG, "vad: on_count + off_count must exceed window");
  PF_CHECK(c.pad_begin >= 0 && c.pad_begin <= 1024 && c.pad_end >= 0 && c.pad_end <= 1024, PF_ERR_INVALID_ARG,
           "vad: pad_begin / pad_end outside 0 .. 1024");
  PF_CHECK((int64_t)c.min_speech >= 2 * (int64_t)std::max(lfr_n, 1), PF_ERR_INVALID_ARG, "vad: min_speech below 2 * lfr_n");
  PF_CHECK(c.split_search >= 0 && c.split_search <= 1024, PF_ERR_INVALID_ARG, "vad: split_search outside 0 .. 1024");
  PF_CHECK(2 * (int64_t)c.min_speech + c.split_search <= (int64_t)c.max_len, PF_ERR_INVALID_ARG,
           "vad: 2 * min_speech + split_search must not exceed max_len");
  return c;
}

void host_vad_levels(const float* rows, int64_t T, int n_mels, int32_t* out) {
  for (int64_t t = 0; t < T; ++t) {
    int32_t e = 0;
    for (int m = 0; m < n_mels; ++m) {
      float v = rows[t * n_mels + m];
      if (!(v > -64.f)) v = -64.f;
      if (v > 64.f) v = 64.f;
      e += (int32_t)rintf(v * 64.f);
    }
    out[t] = e;
  }
}

std::vector<int32_t> host_vad_segments(const int32_t* lev, int T, int n_mels, const pf_vad_config& c) {
  std::vector<int32_t> seg;
  PF_CHECK(T >= 0, PF_ERR_INVALID_ARG, "vad: negative frame count");
  PF_CHECK(T <= PF_VAD_MAX_FRAMES, PF_ERR_CAPACITY, "vad: more than PF_VAD_MAX_FRAMES frames");
  if (T == 0) return seg;
  // 2 threshold
  int64_t thr = c.abs_level;
  if (c.floor_pct >= 0) {
    const int64_t k = std::min<int64_t>(T - 1, (int64_t)T * c.floor_pct / 100);
    std::vector<int32_t> s(lev, lev + T);
    std::nth_element(s.begin(), s.begin() + k, s.end());
    thr = std::max<int64_t>((int64_t)s[(size_t)k] + (int64_t)c.margin_q * n_mels, c.abs_level);
  }
  // 3 window and hysteresis, 4 padding: d[t] through a difference array over the padded frames of every state-1 frame
  std::vector<int32_t> pre((size_t)T + 1, 0), cover((size_t)T + 1, 0);
  for (int t = 0; t < T; ++t) pre[t + 1] = pre[t] + ((int64_t)lev[t] > thr ? 1 : 0);
  int state = 0;
  for (int t = 0; t < T; ++t) {
    const int w = std::min(c.window, t + 1), cnt = pre[t + 1] - pre[t + 1 - w];
    if (cnt >= c.on_count) state = 1;
    else if (w - cnt >= c.off_count) state = 0;
    if (state) { ++cover[std::max(t - c.pad_begin, 0)]; --cover[std::min(t + c.pad_end + 1, T)]; }
  }
  const int64_t max_len = c.max_len;
  auto emit = [&](int64_t b, int64_t e) {
    PF_CHECK(seg.size() / 2 < (size_t)PF_VAD_MAX_SEGMENTS, PF_ERR_CAPACITY, "vad: more than PF_VAD_MAX_SEGMENTS segments");
    seg.push_back((int32_t)b); seg.push_back((int32_t)e);
  };
  int depth = 0, b0 = -1;
  for (int t = 0; t <= T; ++t) {
    depth += t < T ? cover[t] : 0;
    const bool d = t < T && depth > 0;
    if (d && b0 < 0) b0 = t;
    if (!d && b0 >= 0) {
      int64_t b = b0, e = t;
      b0 = -1;
      if (e - b < c.min_speech) continue;
      // 5 split
      while (e - b > max_len) {
        const int64_t hi = std::min(b + max_len, e - c.min_speech), lo = hi - c.split_search;
        int64_t cut = lo;
        for (int64_t x = lo; x <= hi; ++x) if (lev[x] <= lev[cut]) cut = x;
        emit(b, cut);
        b = cut;
      }
      emit(b, e);
    }
  }
  return seg;
}

// ---- streaming endpointing (paraformer_hip.h "Voice-activity endpointing, streaming"; tests/endpoint_ref.py) ----------------
pf_endpoint_config endpoint_default() {
  pf_endpoint_config c{};
  c.struct_size = (int32_t)sizeof(pf_endpoint_config);
  c.rise = 2; c.margin_q = 96; c.abs_level = INT32_MIN;
  c.window = 20; c.on_count = 15; c.off_count = 15;
  c.pad_begin = 30; c.pad_end = 5; c.end_silence = 80;
  c.min_speech = 50; c.max_len = 3000;
  return c;
}

pf_endpoint_config endpoint_check(const pf_endpoint_config* cfg, int lfr_n) {
  if (!cfg) return endpoint_default();
  const pf_endpoint_config c = *cfg;
  PF_CHECK(c.struct_size == (int32_t)sizeof(pf_endpoint_config), PF_ERR_INVALID_ARG, "pf_endpoint_config.struct_size mismatch");
  PF_CHECK(c.rise >= -1 && c.rise <= (1 << 20), PF_ERR_INVALID_ARG, "endpoint: rise outside -1 .. 1 << 20");
  PF_CHECK(c.window >= 1 && c.window <= 256, PF_ERR_INVALID_ARG, "endpoint: window outside 1 .. 256");
  PF_CHECK(c.on_count >= 1 && c.on_count <= c.window && c.off_count >= 1 && c.off_count <= c.window, PF_ERR_INVALID_ARG,
           "endpoint: on_count / off_count outside 1 .. window");
  PF_CHECK(c.on_count + c.off_count > c.window, PF_ERR_INVALID_ARG, "endpoint: on_count + off_count must exceed window");
  PF_CHECK(c.pad_begin >= 0 && c.pad_begin <= 1024, PF_ERR_INVALID_ARG, "endpoint: pad_begin outside 0 .. 1024");
  PF_CHECK(c.end_silence >= 1 && c.end_silence <= (1 << 16), PF_ERR_INVALID_ARG, "endpoint: end_silence outside 1 .. 1 << 16");
  PF_CHECK(c.pad_end >= 0 && c.pad_end <= c.end_silence, PF_ERR_INVALID_ARG, "endpoint: pad_end outside 0 .. end_silence");
  PF_CHECK((int64_t)c.min_speech >= 2 * (int64_t)std::max(lfr_n, 1), PF_ERR_INVALID_ARG, "endpoint: min_speech below 2 * lfr_n");
  PF_CHECK(c.min_speech <= c.max_len && c.max_len <= PF_VAD_MAX_FRAMES, PF_ERR_INVALID_ARG,
           "endpoint: max_len outside min_speech .. PF_VAD_MAX_FRAMES");
  PF_CHECK(c.pad_begin < c.max_len, PF_ERR_INVALID_ARG, "endpoint: pad_begin must be below max_len");
  return c;
}

void endpoint_admit(const int32_t* state, int n_new) {
  PF_CHECK(n_new >= 0, PF_ERR_INVALID_ARG, "endpoint: negative frame count");
  // a block no sequence of calls leaves behind is refused: the walk's integer arithmetic relies on these ranges
  const int32_t count = state[kEpCount];
  const int64_t F = (int64_t)(((uint64_t)(uint32_t)state[kEpFloorHi] << 32) | (uint32_t)state[kEpFloorLo]);
  PF_CHECK(count >= 0 && count <= PF_ENDPOINT_MAX_STREAM_FRAMES && (state[kEpState] | 1) == 1 && (state[kEpFlushed] | 1) == 1 &&
               state[kEpLastOne] >= 0 && state[kEpLastOne] <= count && state[kEpRunFirst] >= 0 && state[kEpRunFirst] <= count &&
               state[kEpPrevEnd] >= 0 && state[kEpPrevEnd] <= count && F >= INT32_MIN && F <= INT32_MAX,
           PF_ERR_INVALID_ARG, "endpoint: not a state block of this detector");
  PF_CHECK(!(state[kEpFlushed] && n_new > 0), PF_ERR_INVALID_ARG, "endpoint: frames after a flush");
  PF_CHECK((int64_t)count + n_new <= PF_ENDPOINT_MAX_STREAM_FRAMES, PF_ERR_CAPACITY,
           "endpoint: more than PF_ENDPOINT_MAX_STREAM_FRAMES frames in one stream");
}

std::vector<int32_t> host_endpoint_update(int32_t* s, const int32_t* lev, int n_new, int flush, int n_mels, const pf_endpoint_config& c,
                                          int32_t* in_speech, int32_t* open_begin) {
  endpoint_admit(s, n_new);
  std::vector<int32_t> ev;
  uint32_t h[8];                                               // the 256-bit window, bit 255 the newest frame
  for (int j = 0; j < 8; ++j) h[j] = (uint32_t)s[kEpHist + j];
  int state = s[kEpState], last_one = s[kEpLastOne] - 1, run_first = s[kEpRunFirst] - 1, prev_end = s[kEpPrevEnd], count = s[kEpCount];
  int64_t F = (int64_t)(((uint64_t)(uint32_t)s[kEpFloorHi] << 32) | (uint32_t)s[kEpFloorLo]);
  const int64_t margin = (int64_t)c.margin_q * n_mels;
  auto begin = [&] { return std::max(prev_end, run_first - c.pad_begin); };
  auto emit = [&](int b, int e, int kind) { ev.push_back(b); ev.push_back(e); ev.push_back(kind); };
  for (int i = 0; i < n_new; ++i) {
    const int t = count;
    const int64_t e = lev[i];
    // 2' the tracked floor
    int64_t thr = c.abs_level;
    if (c.rise >= 0) {
      F = t == 0 ? e : std::min(e, F + c.rise);
      thr = std::max<int64_t>(F + margin, c.abs_level);
    }
    for (int j = 0; j < 7; ++j) h[j] = (h[j] >> 1) | (h[j + 1] << 31);
    h[7] = (h[7] >> 1) | (e > thr ? 0x80000000u : 0u);
    // 3 hysteresis: the newest w frames are the top w bits
    const int w = std::min(c.window, t + 1);
    int cnt = 0;
    for (int k = 0; k < w; ++k) cnt += (int)((h[7 - (k >> 5)] >> (31 - (k & 31))) & 1u);
    if (cnt >= c.on_count) state = 1;
    else if (w - cnt >= c.off_count) state = 0;
    // 4' events
    if (state) {
      if (run_first < 0) run_first = t;
      last_one = t;
    } else if (run_first >= 0 && t == last_one + c.end_silence) {
      const int b = begin(), en = last_one + 1 + c.pad_end;
      if (en - b >= c.min_speech) { emit(b, en, PF_ENDPOINT_SILENCE); prev_end = en; }
      run_first = -1;
    }
    // 5' the forced cut
    if (run_first >= 0 && t + 1 - begin() == c.max_len) {
      emit(begin(), t + 1, PF_ENDPOINT_FORCED);
      prev_end = t + 1;
      if (!state) run_first = -1;
    }
    ++count;
  }
  if (flush && !s[kEpFlushed]) {
    // 6 flush
    if (run_first >= 0) {
      const int b = begin(), en = std::min(count, last_one + 1 + c.pad_end);
      if (en - b >= c.min_speech) { emit(b, en, PF_ENDPOINT_FLUSH); prev_end = en; }
      run_first = -1;
    }
    s[kEpFlushed] = 1;
  }
  for (int j = 0; j < 8; ++j) s[kEpHist + j] = (int32_t)h[j];
  s[kEpState] = state; s[kEpLastOne] = last_one + 1; s[kEpRunFirst] = run_first + 1; s[kEpPrevEnd] = prev_end; s[kEpCount] = count;
  if (c.rise >= 0 && count > 0) { s[kEpFloorLo] = (int32_t)(uint32_t)(uint64_t)F; s[kEpFloorHi] = (int32_t)(uint32_t)((uint64_t)F >> 32); }
  if (in_speech) *in_speech = run_first >= 0 ? 1 : 0;
  if (open_begin) *open_begin = run_first >= 0 ? begin() : -1;
  return ev;
}

int host_long_plan(const int32_t* len, int n, int batch_max, int64_t frame_budget, int32_t* batch, int32_t* row) {
  if (batch_max <= 0) batch_max = 32;
  if (frame_budget <= 0) frame_budget = 96000;
  std::vector<int32_t> order((size_t)n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return len[a] > len[b]; });
  int nb = 0;
  for (int i = 0; i < n;) {
    const int64_t L = len[order[i]];
    int rows = 0;
    do {
      batch[order[i]] = nb; row[order[i]] = rows;
      ++rows; ++i;
    } while (i < n && rows < batch_max && (int64_t)(rows + 1) * L <= frame_budget);
    ++nb;
  }
  return nb;
}

}  // namespace pf
