// Plans from openSMILE configuration files (smilextract_hip -C file.conf): an own reader of the reference's config
// format and a symbolic walk over the component graph that either yields a smilehip_lld_config (+ column names) or says
// which component / option of the graph the fused path cannot express. No reference code runs here.
//
// Format, as the reference's cFileConfigReader reads it (src/core/configManager.cpp:1744-2060 file level, :2170-2560
// instance level): sections "[instance:cType]" (a section may be opened several times), "field = value" lines (the
// instance name may prefix the field), comments = lines starting with ; # % // and everything after // on a line,
// C-style /* */ blocks, "\{path}" includes (tried as given, relative to the top-level file, relative to the including
// file), "\cm[long(short){default}:description]" command-line placeholders (also inside an include path) and
// "\cm[long]" references to an option defined earlier. The component list is the instance[NAME].type = cType entries
// of the [componentInstances:cComponentManager] sections.
#include "conf_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>

namespace smilehip_host {

namespace {

std::string trim(const std::string &s) {
  size_t a = 0, b = s.size();
  while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '\r' || s[a] == '\n')) ++a;
  while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r' || s[b - 1] == '\n')) --b;
  return s.substr(a, b - a);
}
std::string dir_of(const std::string &p) {
  const size_t s = p.find_last_of('/');
  return s == std::string::npos ? std::string(".") : p.substr(0, s);
}
bool file_exists(const std::string &p) {
  std::ifstream f(p);
  return f.good();
}
std::string lower(std::string s) {
  for (char &c : s) c = (char)tolower((unsigned char)c);
  return s;
}

struct Parser {
  ConfFile &out;
  const std::map<std::string, std::string> &cmdline;
  std::string top_dir, err;
  int depth = 0;
  std::string cur_name, cur_type;      // the open section: an include is textual, it continues (and may change) the section
  const ConfCmValue *cm_value = nullptr;   // conf_from_sections: the host's own command-line parser answers (effective value of an option)

  // "\cm[long(short){dflt}:descr]trailing" -> value of the option (command line, else default) + trailing
  bool resolve_cm(const std::string &v, std::string &res) {
    if (v.compare(0, 4, "\\cm[") != 0) { res = v; return true; }
    const size_t end = v.find(']');
    if (end == std::string::npos) { err = "missing ']' in command-line reference '" + v + "'"; return false; }
    const std::string body = v.substr(4, end - 4), trailing = v.substr(end + 1);
    std::string name = body, dflt;
    bool has_dflt = false;
    const size_t colon = body.find(':');
    std::string head = colon == std::string::npos ? body : body.substr(0, colon);
    const size_t br = head.find('{');
    if (br != std::string::npos) {
      const size_t be = head.find('}', br);
      if (be == std::string::npos) { err = "missing '}' in command-line reference '" + v + "'"; return false; }
      dflt = head.substr(br + 1, be - br - 1);
      has_dflt = true;
      head = head.substr(0, br);
    }
    const size_t par = head.find('(');
    name = trim(par == std::string::npos ? head : head.substr(0, par));
    std::string short_name;
    if (par != std::string::npos) {
      const size_t pe = head.find(')', par);
      if (pe != std::string::npos) short_name = trim(head.substr(par + 1, pe - par - 1));
    }
    if (!short_name.empty()) out.cm_short[name] = short_name;
    if (has_dflt && !out.cm_defaults.count(name)) out.cm_defaults[name] = dflt;
    std::string host_val;
    if (cm_value && *cm_value && (*cm_value)(name, host_val)) { res = host_val + trailing; out.cm_used.insert(name); return true; }
    auto it = cmdline.find(name);
    if (it == cmdline.end() && out.cm_short.count(name)) it = cmdline.find(out.cm_short[name]);
    if (it != cmdline.end()) res = it->second + trailing;
    else if (out.cm_defaults.count(name)) res = out.cm_defaults[name] + trailing;
    else { err = "command-line option '" + name + "' is referenced before it is defined"; return false; }
    out.cm_used.insert(name);
    return true;
  }

  ConfInstance &instance(const std::string &name, const std::string &type) {
    for (ConfInstance &i : out.inst)
      if (i.name == name) {
        if (i.type.empty()) i.type = type;
        return i;
      }
    out.inst.push_back(ConfInstance{name, type, {}, false});
    return out.inst.back();
  }

  // one line of a section body or a section header (comments at the start of the line and includes are the caller's business)
  bool body_line(std::string l, const std::string &real) {
      const size_t eol = l.find("//");
      if (eol != std::string::npos) l = trim(l.substr(0, eol));
      if (l.empty()) return true;
      if (l[0] == '[') {
        const size_t c = l.find(':'), e = l.find(']');
        if (c == std::string::npos || e == std::string::npos || c > e) { err = "bad section header '" + l + "' in " + real; return false; }
        cur_name = trim(l.substr(1, c - 1));
        cur_type = trim(l.substr(c + 1, e - c - 1));
        if (cur_type != "cComponentManager") instance(cur_name, cur_type).has_section = true;
        return true;
      }
      const size_t eq = l.find('=');
      if (eq == std::string::npos) { err = "missing '=' in line '" + l + "' of " + real; return false; }
      std::string key = trim(l.substr(0, eq)), val;
      if (!resolve_cm(trim(l.substr(eq + 1)), val)) return false;
      val = trim(val);
      if (cur_name.empty()) { err = "field '" + key + "' outside a section in " + real; return false; }
      if (key.compare(0, cur_name.size() + 1, cur_name + ".") == 0) key = key.substr(cur_name.size() + 1);
      if (cur_type == "cComponentManager") {
        if (key.compare(0, 9, "instance[") == 0) {
          const size_t e = key.find(']');
          if (e != std::string::npos && key.substr(e + 1) == ".type") instance(key.substr(9, e - 9), val);
        }
        return true;                                       // nThreads, printLevelStats ...: the manager's own business
      }
      ConfInstance &ci = instance(cur_name, cur_type);
      bool replaced = false;
      for (auto &kv : ci.opts)
        if (kv.first == key) { kv.second = val; replaced = true; }
      if (!replaced) ci.opts.push_back({key, val});
        return true;
  }

  bool parse_file(const std::string &path, const std::string &parent) {
    if (++depth > 32) { err = "include depth exceeded (loop?) at '" + path + "'"; return false; }
    std::string real;
    for (const std::string &cand : {path, top_dir + "/" + path, dir_of(parent) + "/" + path})
      if (file_exists(cand)) { real = cand; break; }
    if (real.empty()) { err = "cannot open config file '" + path + "'"; return false; }
    std::ifstream f(real);
    std::string line;
    bool in_block_comment = false;
    while (std::getline(f, line)) {
      std::string l = trim(line);
      if (in_block_comment) {
        const size_t e = l.find("*/");
        if (e == std::string::npos) continue;
        l = trim(l.substr(e + 2));
        in_block_comment = false;
      }
      if (l.compare(0, 2, "/*") == 0) {
        if (l.find("*/", 2) == std::string::npos) in_block_comment = true;
        continue;
      }
      if (l.empty() || l[0] == ';' || l[0] == '#' || l[0] == '%' || l.compare(0, 2, "//") == 0) continue;
      if (l.size() > 3 && l[0] == '\\' && l[1] == '{' && l.back() == '}') {               // include
        std::string inc;
        if (!resolve_cm(l.substr(2, l.size() - 3), inc)) return false;
        if (!parse_file(inc, real)) return false;
        continue;
      }
      if (!body_line(l, real)) return false;
    }
    --depth;
    return true;
  }
};

bool is_io_type(const std::string &t) {
  return t == "cDataMemory" || t == "cWaveSource" || t == "cComponentManager" || (t.size() > 4 && t.compare(t.size() - 4, 4, "Sink") == 0);
}

std::string canonical_value(const std::string &v) {
  char *end = nullptr;
  const double d = strtod(v.c_str(), &end);
  if (end != v.c_str() && *end == 0) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.17g", d);
    return buf;
  }
  return v;
}

// ---- symbolic columns of a data-memory level of the cepstral chains
struct Col {
  int kind;        // 0 cepstrum, 1 log energy
  int index;       // cepstrum number as the component names it
  int delta;       // order of delta regression applied
  bool cms;        // cFullinputMean applied (before any delta)
};

struct OptReader {
  const ConfInstance &ci;
  std::set<std::string> seen;
  std::string err;
  explicit OptReader(const ConfInstance &c) : ci(c) {}
  bool has(const std::string &k) const { return ci.find(k) != nullptr; }
  std::string str(const std::string &k, const std::string &d) {
    seen.insert(k);
    const std::string *v = ci.find(k);
    return v ? *v : d;
  }
  double num(const std::string &k, double d) {
    seen.insert(k);
    const std::string *v = ci.find(k);
    if (!v) return d;
    char *end = nullptr;
    const double x = strtod(v->c_str(), &end);
    if (end == v->c_str()) { err = "[" + ci.name + ":" + ci.type + "] " + k + " = '" + *v + "' is not a number"; return d; }
    return x;
  }
  // option must have this value (given or by default)
  bool require(const std::string &k, double want, double dflt) {
    const double x = num(k, dflt);
    if (x != want && err.empty()) {
      std::ostringstream o;
      o << "[" << ci.name << ":" << ci.type << "] " << k << " = " << x << " is not expressible on the fused path (needs " << want << ")";
      err = o.str();
    }
    return err.empty();
  }
  // every option of the section must have been looked at, or be one of the benign ones
  bool finish(const std::set<std::string> &benign) {
    if (!err.empty()) return false;
    for (const auto &kv : ci.opts) {
      if (seen.count(kv.first) || benign.count(kv.first)) continue;
      if (kv.first.compare(0, 17, "writer.levelconf.") == 0 || kv.first.compare(0, 17, "reader.levelconf.") == 0) continue;
      err = "[" + ci.name + ":" + ci.type + "] option '" + kv.first + "' is not expressible on the fused path";
      return false;
    }
    return true;
  }
};

const std::set<std::string> kBenign = {"reader.dmLevel", "writer.dmLevel", "copyInputName", "buffersize", "buffersize_sec", "blocksize",
                                       "blocksizeR", "blocksizeW", "blocksize_sec", "blocksizeR_sec", "blocksizeW_sec", "EOIlevel"};

int win_func_of(const std::string &w) {
  const std::string s = lower(w);
  if (s == "han" || s == "hann" || s == "hanning") return SMILEHIP_WIN_HANN;
  if (s == "ham" || s == "hamming") return SMILEHIP_WIN_HAMM;
  if (s == "rec" || s == "rectangular" || s == "none") return SMILEHIP_WIN_RECT;
  if (s == "gau" || s == "gauss" || s == "gaussian") return SMILEHIP_WIN_GAUSS;
  if (s == "sin" || s == "sine" || s == "cos" || s == "cosine") return SMILEHIP_WIN_SINE;
  if (s == "tri" || s == "triangle") return SMILEHIP_WIN_TRI;
  if (s == "bar" || s == "bartlett") return SMILEHIP_WIN_BARTLETT;
  if (s == "lac" || s == "lanczos") return SMILEHIP_WIN_LANCZOS;
  return -1;
}

std::vector<std::string> split_levels(const std::string &s) {
  std::vector<std::string> r;
  std::stringstream ss(s);
  std::string item;
  while (std::getline(ss, item, ';'))
    if (!trim(item).empty()) r.push_back(trim(item));
  return r;
}

}  // namespace

const std::string *ConfInstance::find(const std::string &key) const {
  for (const auto &kv : opts)
    if (kv.first == key) return &kv.second;
  return nullptr;
}

bool conf_parse(const std::string &path, const std::map<std::string, std::string> &cmdline, ConfFile &out, std::string &err) {
  out = ConfFile();
  Parser p{out, cmdline, dir_of(path), "", 0, "", ""};
  if (!p.parse_file(path, path)) { err = p.err; return false; }
  for (const ConfInstance &i : out.inst)
    if (i.type.empty()) { err = "instance '" + i.name + "' has no type"; return false; }
  return true;
}

bool conf_from_sections(const std::vector<ConfRawSection> &sections, const ConfCmValue &cm_value, ConfFile &out, std::string &err) {
  out = ConfFile();
  static const std::map<std::string, std::string> none;
  Parser p{out, none, ".", "", 0, "", ""};
  p.cm_value = &cm_value;
  for (const ConfRawSection &sec : sections) {
    p.cur_name = sec.name;
    p.cur_type = sec.type;
    if (sec.type != "cComponentManager") p.instance(sec.name, sec.type).has_section = true;
    for (const std::string &raw : sec.lines) {
      const std::string l = trim(raw);
      if (l.empty() || l[0] == ';' || l[0] == '#' || l[0] == '%' || l.compare(0, 2, "//") == 0) continue;
      if (!p.body_line(l, "(configuration manager)")) { err = p.err; return false; }
    }
  }
  for (const ConfInstance &i : out.inst)
    if (i.type.empty()) { err = "instance '" + i.name + "' has no type"; return false; }
  return true;
}

// FNV-1a over the processing components (sources, sinks and the data memory left out: they follow the command line),
// sections in instantiation order, options sorted, numbers in canonical form
uint64_t conf_fingerprint(const ConfFile &f) {
  uint64_t h = 1469598103934665603ull;
  auto eat = [&](const std::string &s) {
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    h ^= '\n'; h *= 1099511628211ull;
  };
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    eat(i.name + ":" + i.type);
    std::vector<std::pair<std::string, std::string>> o = i.opts;
    std::sort(o.begin(), o.end());
    for (const auto &kv : o) eat(kv.first + "=" + canonical_value(kv.second));
  }
  return h;
}

// The options of the F0 group the chains take as parameters (smilehip_lld_config fields): cPitchShs (pitchShs.cpp /
// pitchBase.cpp options), cPitchSmootherViterbi bufferLength, cPitchJitter searchRangeRel / useBrokenJitterThresh and the
// threshold of the energy gate ([is13_volmerge] / [gemapsv01b_volmerge]). Returns the config field's name, or nullptr.
static const char *conf_is_f0_param(const ConfInstance &i, const std::string &key) {
  if (i.type == "cPitchShs") {
    if (key == "minPitch") return "pitch_min";
    if (key == "maxPitch") return "pitch_max";
    if (key == "voicingCutoff") return "voicing_cutoff";
    if (key == "nHarmonics") return "shs_n_harmonics";
    if (key == "compressionFactor") return "shs_compression";
  }
  if (i.type == "cPitchSmootherViterbi" && key == "bufferLength") return "vit_buffer_len";
  if (i.type == "cPitchJitter") {
    if (key == "searchRangeRel") return "jitter_search_range";
    if (key == "useBrokenJitterThresh") return "jitter_broken_thresh";
  }
  if (i.type == "cValbasedSelector" && key == "threshold" && i.name.size() >= 8 && i.name.compare(i.name.size() - 8, 8, "volmerge") == 0)
    return "f0_min_energy";
  return nullptr;
}

uint64_t conf_fingerprint_masked(const ConfFile &f) {
  uint64_t h = 1469598103934665603ull;
  auto eat = [&](const std::string &s) {
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    h ^= '\n'; h *= 1099511628211ull;
  };
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    eat(i.name + ":" + i.type);
    std::vector<std::pair<std::string, std::string>> o = i.opts;
    std::sort(o.begin(), o.end());
    // a parameter's VALUE is masked, its presence is not: a file that leaves the line out gets the component's own default
    // from the reference (pitchJitter.cpp:47/77, pitchSmootherViterbi.cpp:42 ...), not the shipped file's value
    for (const auto &kv : o)
      eat(conf_is_f0_param(i, kv.first) ? kv.first + "=<parameter>" : kv.first + "=" + canonical_value(kv.second));
  }
  return h;
}

static bool conf_is_selection_param(const ConfInstance &i, const std::string &key) {
  return (i.type == "cMfcc" && key == "lastMfcc") || (i.type == "cFunctionals" && key == "functionalsEnabled");
}
uint64_t conf_fingerprint_masked2(const ConfFile &f) {
  uint64_t h = 1469598103934665603ull;
  auto eat = [&](const std::string &s) {
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    h ^= '\n'; h *= 1099511628211ull;
  };
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    eat(i.name + ":" + i.type);
    std::vector<std::pair<std::string, std::string>> o = i.opts;
    std::sort(o.begin(), o.end());
    for (const auto &kv : o)
      eat((conf_is_f0_param(i, kv.first) || conf_is_selection_param(i, kv.first)) ? kv.first + "=<parameter>"
                                                                                  : kv.first + "=" + canonical_value(kv.second));
  }
  return h;
}

void conf_apply_f0_params(const ConfPlan &p, smilehip_lld_config &c) {
  for (const auto &kv : p.f0_params) {
    if (kv.first == "pitch_min") c.pitch_min = kv.second;
    else if (kv.first == "pitch_max") c.pitch_max = kv.second;
    else if (kv.first == "voicing_cutoff") c.voicing_cutoff = kv.second;
    else if (kv.first == "shs_n_harmonics") c.shs_n_harmonics = (int32_t)kv.second;
    else if (kv.first == "shs_compression") c.shs_compression = (float)kv.second;
    else if (kv.first == "vit_buffer_len") c.vit_buffer_len = (int32_t)kv.second;
    else if (kv.first == "jitter_search_range") c.jitter_search_range = kv.second;
    else if (kv.first == "jitter_broken_thresh") c.jitter_broken_thresh = (int32_t)kv.second;
    else if (kv.first == "f0_min_energy") c.f0_min_energy = (float)kv.second;
    else if (kv.first == "shs_n_candidates") c.shs_n_candidates = (int32_t)kv.second;
    else if (kv.first == "specscale_min_f") c.specscale_min_f = kv.second;
    else if (kv.first == "sma_win") c.sma_win = (int32_t)kv.second;
    else if (kv.first == "tonespec_n_octaves") c.tonespec_n_octaves = (int32_t)kv.second;
    else if (kv.first == "tonespec_first_note") c.tonespec_first_note = (float)kv.second;
    else if (kv.first == "tonespec_filter_type") c.tonespec_filter_type = (int32_t)kv.second;
    else if (kv.first == "tonespec_use_power") c.tonespec_use_power = (int32_t)kv.second;
    else if (kv.first == "tonespec_dba") c.tonespec_dba = (int32_t)kv.second;
    else if (kv.first == "chroma_octave_size") c.chroma_octave_size = (int32_t)kv.second;
    else if (kv.first == "chroma_sil_thresh") c.chroma_sil_thresh = (float)kv.second;
    else if (kv.first == "tonefilt_n_notes") c.tonefilt_n_notes = (int32_t)kv.second;
    else if (kv.first == "tonefilt_first_note") c.tonefilt_first_note = kv.second;
    else if (kv.first == "tonefilt_decay_f0") c.tonefilt_decay_f0 = kv.second;
    else if (kv.first == "tonefilt_decay_fn") c.tonefilt_decay_fn = kv.second;
    else if (kv.first == "tonefilt_output_period") c.tonefilt_output_period = c.frame_size_sec = c.frame_step_sec = kv.second;   // (the block is the plan's frame)
  }
}

namespace {
struct KnownSet { uint64_t fingerprint; const char *set; const char *file; uint64_t masked; uint64_t masked2 = 0; };
// fingerprints of the reference's own files (smilextract_hip -C <file> --fingerprint prints them), computed from
// config/is09-13/IS09_emotion.conf, config/compare16/ComParE_2016.conf, config/is09-13/IS13_ComParE.conf and
// config/egemaps/v02/eGeMAPSv02.conf (and its two sub-graphs, GeMAPSv01b.conf / eGeMAPSv01b.conf) with their includes and every command-line option at its default
const KnownSet kKnownSets[] = {
    {0x84b42d91f07908acull, "is09_emotion", "IS09_emotion.conf", 0},
    {0x9c0cc5d423cf1caeull, "compare16", "ComParE_2016.conf", 0xfae69d014d0dfa60ull, 0x4f1f91fabefddeebull},
    {0xb409f82a744a62d2ull, "is13_compare", "IS13_ComParE.conf", 0x5a6b988a3b68a67full, 0xfe35c75d8b8a8138ull},
    {0xcb39106ceca6480cull, "egemapsv02", "eGeMAPSv02.conf", 0xb17c462e03023f64ull},
    // sub-graphs of eGeMAPSv02.conf: their levels are column subsets of its levels (smilehip_host.hpp, egemaps_subset_columns)
    {0x07901132e1b570f7ull, "gemapsv01b", "GeMAPSv01b.conf", 0xc9092680fbe30c4full},
    {0xe0e523408610f510ull, "egemapsv01b", "eGeMAPSv01b.conf", 0x3cde1ce6e1776678ull},
    // the v01a files: the same sub-graphs with zeroPadSymmetric = 0, useBrokenJitterThresh = 1, maxF = 5500 (smilehip_config_egemapsv01a)
    {0x54c6dceabc3deb6full, "gemapsv01a", "GeMAPSv01a.conf", 0x20e46a265c0b88beull},
    {0x378e8dfc3678ce85ull, "egemapsv01a", "eGeMAPSv01a.conf", 0x6956ca30c993252cull},
};
}  // namespace

bool conf_check_io(const ConfFile &f, const std::set<std::string> &produced, std::string &err, bool values_only_csv) {
  auto num_is = [](const std::string &v, double want) {
    char *end = nullptr;
    const double d = strtod(v.c_str(), &end);
    return end != v.c_str() && d == want;
  };
  for (const ConfInstance &i : f.inst) {
    if (i.type == "cWaveSource") {
      // waveSource.cpp:52-68: the fused path packs whole files
      static const std::pair<const char *, double> whole[] = {{"start", 0}, {"end", -1}, {"endrel", 0}, {"startSamples", 0},
                                                               {"endSamples", -1}, {"endrelSamples", 0}, {"noHeader", 0}};
      for (const auto &w : whole) {
        const std::string *v = i.find(w.first);
        if (v && !num_is(*v, w.second)) {
          err = "[" + i.name + ":cWaveSource] " + w.first + " = " + *v + ": the fused path reads whole files (only " + w.first + " = " +
                canonical_value(std::to_string(w.second)) + " is implemented)";
          return false;
        }
      }
      const std::string *seg = i.find("segmentList");
      if (seg && !seg->empty()) { err = "[" + i.name + ":cWaveSource] segmentList is not implemented by the fused path"; return false; }
      continue;
    }
    const bool sink = i.type.size() > 4 && i.type.compare(i.type.size() - 4, 4, "Sink") == 0;
    if (!sink) continue;
    const std::string *fn = i.find("filename");
    if (!fn || *fn == "?") continue;                       // a disabled sink (the shared output files' default)
    if (i.type != "cHtkSink" && i.type != "cCsvSink" && i.type != "cArffSink") {
      err = "[" + i.name + ":" + i.type + "] is active (filename = " + *fn + ") but smilextract_hip has no writer for it";
      return false;
    }
    const std::string *lv = i.find("reader.dmLevel");
    if (lv && !produced.empty()) {
      size_t a = 0;
      while (a <= lv->size()) {                            // "lld;lld_de": every level the sink reads
        const size_t b = lv->find(';', a);
        const std::string one = lv->substr(a, b == std::string::npos ? std::string::npos : b - a);
        if (!one.empty() && !produced.count(one)) {
          err = "[" + i.name + ":" + i.type + "] reads level '" + one + "', which the fused path does not write (it keeps only the "
                "output levels; intermediate levels: per-component operators through the plugin)";
          return false;
        }
        if (b == std::string::npos) break;
        a = b + 1;
      }
    }
    const bool on_func = lv && *lv == "func";
    // The values the sink would run with -- the option if the file sets it, else the component's own default (csvSink.cpp:43-51,
    // 95-104; arffSink.cpp:42-51, 104-120; htkSink.cpp:33-37), `frameIndex` / `frameTime` overriding their synonyms `number` /
    // `timestamp` when set -- against the one value the writers of opensmile_amd/host/sinks.cpp implement for this kind of sink.
    auto value_of = [&](const char *key, double dflt, bool &bad) {
      const std::string *v = i.find(key);
      if (!v) return dflt;
      char *end = nullptr;
      const double d = strtod(v->c_str(), &end);
      if (end == v->c_str()) { bad = true; return dflt; }
      return d;
    };
    // what the file asks of a sink option against what smilextract_hip's writers do: `was_set` = the file names the option (under
    // either of its spellings), `exact` = the value itself must match (offsets), not only its being zero or not (switches)
    struct Want { const char *what; double has; double implemented; bool was_set; bool exact; };
    std::vector<Want> wants;
    bool bad = false;
    const auto set = [&](const char *a, const char *b = nullptr) { return i.find(a) != nullptr || (b && i.find(b) != nullptr); };
    const double number = i.find("frameIndex") ? value_of("frameIndex", 1, bad) : value_of("number", 1, bad);
    const double stamp = i.find("frameTime") ? value_of("frameTime", 1, bad) : value_of("timestamp", 1, bad);
    const bool number_set = set("frameIndex", "number"), stamp_set = set("frameTime", "timestamp");
    const auto plain = [&](const char *key, double dflt, double implemented, bool exact = false) {
      return Want{key, value_of(key, dflt, bad), implemented, set(key), exact};
    };
    if (i.type == "cCsvSink")
      wants = {{"timestamp / frameTime", stamp, values_only_csv ? 0.0 : 1.0, stamp_set, false}, plain("printHeader", 1, values_only_csv ? 0 : 1),
               {"number / frameIndex", number, 0, number_set, false},
               plain("frameLength", 0, 0), plain("lag", 0, 0, true), plain("append", 0, on_func ? 1.0 : 0.0)};
    if (i.type == "cArffSink")
      wants = {{"number / frameIndex", number, 0, number_set, false}, {"timestamp / frameTime", stamp, on_func ? 0.0 : 1.0, stamp_set, false},
               plain("frameTimeAdd", 0, 0, true), plain("frameLength", 0, 0), plain("lag", 0, 0, true), plain("append", 0, 1)};
    if (i.type == "cHtkSink") wants = {plain("append", 0, 0), plain("lag", 0, 0, true)};
    if (bad) { err = "[" + i.name + ":" + i.type + "] has a numeric option that does not parse"; return false; }
    for (const Want &w : wants)
      if (w.exact ? w.has != w.implemented : (w.has != 0) != (w.implemented != 0)) {
        err = "[" + i.name + ":" + i.type + "] " + w.what + " = " + canonical_value(std::to_string(w.has)) + (w.was_set ? "" : " (the component's default where the file is silent)") +
              " is not implemented by smilextract_hip's writer (only " + canonical_value(std::to_string(w.implemented)) + ")";
        return false;
      }
    if (i.type == "cArffSink" && !on_func) {
      err = "[" + i.name + ":cArffSink] an ARFF file of the LLD level (-lldarffoutput) is not implemented by smilextract_hip";
      return false;
    }
    const std::string *delim = i.find("delimChar");
    if (delim && *delim != ";") { err = "[" + i.name + ":cCsvSink] delimChar = " + *delim + " is not implemented (only ';')"; return false; }
  }
  return true;
}

// ---- smilextract_hip --set prosody_shs -C file: config/prosody/prosodyShs.conf, possibly with other values of the options the chain takes as
// parameters. (Plain -C does not map the file: conf_to_plan is unchanged.) The graph is walked component by
// component, every option either has the one value SMILEHIP_CHAIN_PROSODY_SHS implements or is one of its parameters (cPitchShs
// minPitch, maxPitch, voicingCutoff, nHarmonics, compressionFactor, nCandidates; cSpecScale minF; cContourSmoother smaWin)
// fingerprint of the reference's own file with its includes and every command-line option at its default (--fingerprint prints it)
static const uint64_t kProsodyShsFingerprint = 0xbb9ed3ae4574db3cull;
static const std::set<std::string> kProsodyTypes = {"cFramer", "cIntensity", "cWindower", "cTransformFFT", "cFFTmagphase", "cSpecScale",
                                                    "cPitchShs", "cPitchSmoother", "cContourSmoother"};
bool conf_to_prosody_shs(const ConfFile &f, ConfPlan &p, std::string &err) {
  p = ConfPlan();
  std::map<std::string, const ConfInstance *> one;
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    if (!kProsodyTypes.count(i.type)) { err = "component [" + i.name + ":" + i.type + "] is not part of the graph of prosodyShs.conf"; return false; }
    if (one.count(i.type)) { err = "more than one " + i.type + " ([" + i.name + "]): not the graph of prosodyShs.conf"; return false; }
    one[i.type] = &i;
  }
  for (const std::string &t : kProsodyTypes)
    if (!one.count(t)) { err = "the graph has no " + t + ": not the graph of prosodyShs.conf"; return false; }
  auto lvl = [](const ConfInstance *i, const char *k) { const std::string *v = i->find(k); return v ? *v : std::string(); };
  auto wired = [&](const ConfInstance *i, const std::string &want) {
    if (lvl(i, "reader.dmLevel") == want) return true;
    err = "[" + i->name + ":" + i->type + "] reader.dmLevel = '" + lvl(i, "reader.dmLevel") + "', expected '" + want + "' (not the wiring of prosodyShs.conf)";
    return false;
  };
  auto must_be = [](OptReader &o, const char *key, const char *want, const char *dflt) {
    const std::string v = o.str(key, dflt);
    if (lower(v) != lower(want) && o.err.empty())
      o.err = "[" + o.ci.name + ":" + o.ci.type + "] " + key + " = " + v + " is not expressible on the fused path (needs " + want + ")";
  };
  const ConfInstance *fr = one["cFramer"], *in = one["cIntensity"], *win = one["cWindower"], *fft = one["cTransformFFT"],
                     *mag = one["cFFTmagphase"], *sc = one["cSpecScale"], *shs = one["cPitchShs"], *sm = one["cPitchSmoother"],
                     *smo = one["cContourSmoother"];
  {                                                       // src/core/winToVecProcessor.cpp:51-83
    OptReader o(*fr);
    if (!wired(fr, "wave")) return false;
    o.require("frameSize", 0.05, 0.025); o.require("frameStep", 0.01, 0.0);
    must_be(o, "frameMode", "fixed", "fixed"); must_be(o, "frameCenterSpecial", "left", "left");
    o.require("noPostEOIprocessing", 1, 1); o.require("frameSizeFrames", 0, 0); o.require("frameStepFrames", 0, 0);
    o.require("frameCenter", 0, 0); o.require("frameCenterFrames", 0, 0); o.require("allowLastFrameIncomplete", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  const std::string frames = lvl(fr, "writer.dmLevel");
  {                                                       // src/lldcore/intensity.cpp:36-38
    OptReader o(*in);
    if (!wired(in, frames)) return false;
    o.require("intensity", 0, 1); o.require("loudness", 1, 0); o.require("processArrayFields", 1, 1);
    if (o.has("nameAppend") && !o.str("nameAppend", "").empty()) o.err = "[" + in->name + ":cIntensity] nameAppend is not expressible on the fused path (needs none)";
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/windower.cpp:36-49
    OptReader o(*win);
    if (!wired(win, frames)) return false;
    const std::string wf = o.str("winFunc", "Han");
    if (win_func_of(wf) != SMILEHIP_WIN_GAUSS) o.err = "[" + win->name + ":cWindower] winFunc = " + wf + " is not expressible on the fused path (needs gauss)";
    o.require("gain", 1, 1); o.require("sigma", 0.4, 0.4); o.require("offset", 0, 0);
    o.require("fade", 0, 0); o.require("squareRoot", 0, 0); o.require("xshift", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/transformFft.cpp:34-35
    OptReader o(*fft);
    if (!wired(fft, lvl(win, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0); o.require("zeroPadSymmetric", 0, 1); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/fftmagphase.cpp:39-49
    OptReader o(*mag);
    if (!wired(mag, lvl(fft, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0); o.require("magnitude", 1, 1); o.require("phase", 0, 0); o.require("joinMagphase", 0, 0);
    o.require("normalise", 0, 0); o.require("power", 0, 0); o.require("dBpsd", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dsp/specScale.cpp:44-73
    OptReader o(*sc);
    if (!wired(sc, lvl(mag, "writer.dmLevel"))) return false;
    must_be(o, "scale", "octave", "log"); must_be(o, "sourceScale", "lin", "lin"); must_be(o, "interpMethod", "spline", "spline");
    const double min_f = o.num("minF", 25.0);
    if (!(min_f > 0.0) && o.err.empty()) o.err = "[" + sc->name + ":cSpecScale] minF = " + canonical_value(std::to_string(min_f)) + " is not expressible on the fused path (needs > 0)";
    p.f0_params["specscale_min_f"] = min_f;
    o.require("maxF", -1, -1); o.require("nPointsTarget", 0, 0); o.require("specSmooth", 1, 0); o.require("specEnhance", 1, 0);
    o.require("auditoryWeighting", 1, 0); o.require("processArrayFields", 0, 0);
    o.num("logScaleBase", 2.0); o.num("logSourceScaleBase", 2.0); o.num("firstNote", 55.0);   // (not read with scale = octave, sourceScale = lin)
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lldcore/pitchBase.cpp:41-60, src/lld/pitchShs.cpp:55-62
    OptReader o(*shs);
    if (!wired(shs, lvl(sc, "writer.dmLevel"))) return false;
    p.f0_params["pitch_max"] = o.num("maxPitch", 620.0);
    p.f0_params["pitch_min"] = o.num("minPitch", 52.0);
    p.f0_params["voicing_cutoff"] = o.num("voicingCutoff", 0.70);
    p.f0_params["shs_n_harmonics"] = o.num("nHarmonics", 15);
    p.f0_params["shs_compression"] = o.num("compressionFactor", 0.85);
    const double nc = o.num("nCandidates", 3);
    if ((nc < 1 || nc > 6 || nc != std::floor(nc)) && o.err.empty())
      o.err = "[" + shs->name + ":cPitchShs] nCandidates = " + canonical_value(std::to_string(nc)) + " is not expressible on the fused path (needs 1 .. 6)";
    p.f0_params["shs_n_candidates"] = nc;
    o.require("scores", 1, 1); o.require("voicing", 1, 1); o.require("F0C1", 0, 0); o.require("voicingC1", 0, 0); o.require("F0raw", 1, 0);
    o.require("voicingClip", 1, 0); o.require("octaveCorrection", 0, 0); o.require("greedyPeakAlgo", 0, 0); o.require("shsSpectrumOutput", 0, 0);
    o.require("lfCut", 0, 0); o.require("processArrayFields", 0, 0);
    must_be(o, "inputFieldSearch", "Mag_logScale", "Mag_logScale");
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lldcore/pitchSmoother.cpp:39-57
    OptReader o(*sm);
    if (!wired(sm, lvl(shs, "writer.dmLevel"))) return false;
    o.require("medianFilter0", 0, 0); o.require("postSmoothing", 0, 0); must_be(o, "postSmoothingMethod", "simple", "simple");
    o.require("octaveCorrection", 0, 1); o.require("F0final", 1, 1); o.require("F0finalEnv", 0, 0); o.require("no0f0", 0, 0);
    o.require("voicingFinalClipped", 0, 0); o.require("voicingFinalUnclipped", 1, 0); o.require("F0raw", 0, 0); o.require("voicingC1", 0, 0);
    o.require("voicingClip", 0, 0); o.require("processArrayFields", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/contourSmoother.cpp:33-36, src/core/windowProcessor.cpp:39
    OptReader o(*smo);
    if (!wired(smo, lvl(sm, "writer.dmLevel") + ";" + lvl(in, "writer.dmLevel"))) return false;
    const double w = o.num("smaWin", 3);
    if ((w < 3 || w > 9 || w != std::floor(w) || !((int)w & 1)) && o.err.empty())
      o.err = "[" + smo->name + ":cContourSmoother] smaWin = " + canonical_value(std::to_string(w)) + " is not expressible on the fused path (needs an odd number, 3 .. 9)";
    p.f0_params["sma_win"] = w;
    o.require("noZeroSma", 0, 0); o.require("noPostEOIprocessing", 0, 0);
    must_be(o, "nameAppend", "sma", "sma");
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  if (lvl(smo, "writer.dmLevel") != "lld") {
    err = "[" + smo->name + ":cContourSmoother] writer.dmLevel = '" + lvl(smo, "writer.dmLevel") + "', expected 'lld' (the level the shared output file's sinks read)";
    return false;
  }
  if (!conf_check_io(f, {"lld"}, err)) return false;
  p.preset = "prosody_shs";
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
  if (conf_fingerprint(f) == kProsodyShsFingerprint) {     // the shipped file: the preset as it is
    p.f0_params.clear();
    p.describe = "the graph of prosodyShs.conf (every processing component and option identical)";
    return true;
  }
  std::string what;
  for (const auto &kv : p.f0_params) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%s%s = %.9g", what.empty() ? "" : ", ", kv.first.c_str(), kv.second);
    what += buf;
  }
  p.describe = "the graph of prosodyShs.conf with the file's own parameter values (" + what + ")";
  return true;
}

// ---- smilextract_hip --set prosody_acf -C file: config/prosody/prosodyAcf.conf, possibly with other values of the options the chain
// takes as parameters (cPitchACF maxPitch, voicingCutoff; cContourSmoother smaWin). Walked like prosodyShs.conf above: every other
// option has the one value SMILEHIP_CHAIN_PROSODY_ACF implements or is refused by name. (Plain -C does not map the file.)
// fingerprint of the reference's own file with its includes and every command-line option at its default (--fingerprint prints it)
static const uint64_t kProsodyAcfFingerprint = 0xe34c269f6b709ce4ull;
bool conf_to_prosody_acf(const ConfFile &f, ConfPlan &p, std::string &err) {
  p = ConfPlan();
  static const std::set<std::string> types = {"cFramer", "cIntensity", "cWindower", "cTransformFFT", "cFFTmagphase", "cAcf", "cPitchACF",
                                              "cContourSmoother"};
  std::map<std::string, const ConfInstance *> one;
  std::vector<const ConfInstance *> acfs;
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    if (!types.count(i.type)) { err = "component [" + i.name + ":" + i.type + "] is not part of the graph of prosodyAcf.conf"; return false; }
    if (i.type == "cAcf") { acfs.push_back(&i); continue; }
    if (one.count(i.type)) { err = "more than one " + i.type + " ([" + i.name + "]): not the graph of prosodyAcf.conf"; return false; }
    one[i.type] = &i;
  }
  for (const std::string &t : types)
    if (t != "cAcf" && !one.count(t)) { err = "the graph has no " + t + ": not the graph of prosodyAcf.conf"; return false; }
  if (acfs.size() != 2) { err = "the graph has " + std::to_string(acfs.size()) + " cAcf instances, prosodyAcf.conf has two (ACF and cepstrum)"; return false; }
  auto lvl = [](const ConfInstance *i, const char *k) { const std::string *v = i->find(k); return v ? *v : std::string(); };
  auto wired = [&](const ConfInstance *i, const std::string &want) {
    if (lvl(i, "reader.dmLevel") == want) return true;
    err = "[" + i->name + ":" + i->type + "] reader.dmLevel = '" + lvl(i, "reader.dmLevel") + "', expected '" + want + "' (not the wiring of prosodyAcf.conf)";
    return false;
  };
  auto must_be = [](OptReader &o, const char *key, const char *want, const char *dflt) {
    const std::string v = o.str(key, dflt);
    if (lower(v) != lower(want) && o.err.empty())
      o.err = "[" + o.ci.name + ":" + o.ci.type + "] " + key + " = " + v + " is not expressible on the fused path (needs " + want + ")";
  };
  const ConfInstance *fr = one["cFramer"], *in = one["cIntensity"], *win = one["cWindower"], *fft = one["cTransformFFT"],
                     *mag = one["cFFTmagphase"], *pit = one["cPitchACF"], *smo = one["cContourSmoother"];
  // which cAcf is which: cPitchACF reads "<acf level>;<cepstrum level>" (pitchACF.cpp:148-164: the ACF first)
  const std::vector<std::string> pin = split_levels(lvl(pit, "reader.dmLevel"));
  const ConfInstance *acf = nullptr, *cep = nullptr;
  if (pin.size() == 2)
    for (const ConfInstance *a : acfs) {
      if (lvl(a, "writer.dmLevel") == pin[0] && !acf) acf = a;
      else if (lvl(a, "writer.dmLevel") == pin[1] && !cep) cep = a;
    }
  if (!acf || !cep) {
    err = "[" + pit->name + ":cPitchACF] reader.dmLevel = '" + lvl(pit, "reader.dmLevel") + "', expected the levels of the two cAcf instances, ACF first (not the wiring of prosodyAcf.conf)";
    return false;
  }
  {                                                       // the cepstrum instance where the ACF belongs (and the other way round): the reader's order
    const std::string *ca = acf->find("cepstrum"), *cc = cep->find("cepstrum");
    if (ca && atof(ca->c_str()) != 0.0 && !(cc && atof(cc->c_str()) != 0.0)) {
      err = "[" + pit->name + ":cPitchACF] reader.dmLevel = '" + lvl(pit, "reader.dmLevel") + "' names the cepstrum's level first; cPitchACF takes the ACF first (not the wiring of prosodyAcf.conf)";
      return false;
    }
  }
  {                                                       // src/core/winToVecProcessor.cpp:51-83
    OptReader o(*fr);
    if (!wired(fr, "wave")) return false;
    o.require("frameSize", 0.05, 0.025); o.require("frameStep", 0.01, 0.0);
    must_be(o, "frameMode", "fixed", "fixed"); must_be(o, "frameCenterSpecial", "left", "left");
    o.require("noPostEOIprocessing", 1, 1); o.require("frameSizeFrames", 0, 0); o.require("frameStepFrames", 0, 0);
    o.require("frameCenter", 0, 0); o.require("frameCenterFrames", 0, 0); o.require("allowLastFrameIncomplete", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  const std::string frames = lvl(fr, "writer.dmLevel");
  {                                                       // src/lldcore/intensity.cpp:36-38
    OptReader o(*in);
    if (!wired(in, frames)) return false;
    o.require("intensity", 0, 1); o.require("loudness", 1, 0); o.require("processArrayFields", 1, 1);
    if (o.has("nameAppend") && !o.str("nameAppend", "").empty()) o.err = "[" + in->name + ":cIntensity] nameAppend is not expressible on the fused path (needs none)";
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/windower.cpp:36-49
    OptReader o(*win);
    if (!wired(win, frames)) return false;
    const std::string wf = o.str("winFunc", "Han");
    if (win_func_of(wf) != SMILEHIP_WIN_GAUSS) o.err = "[" + win->name + ":cWindower] winFunc = " + wf + " is not expressible on the fused path (needs gauss)";
    o.require("gain", 1, 1); o.require("sigma", 0.4, 0.4); o.require("offset", 0, 0);
    o.require("fade", 0, 0); o.require("squareRoot", 0, 0); o.require("xshift", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/transformFft.cpp:34-35
    OptReader o(*fft);
    if (!wired(fft, lvl(win, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0); o.require("zeroPadSymmetric", 0, 1); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/fftmagphase.cpp:39-49
    OptReader o(*mag);
    if (!wired(mag, lvl(fft, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0); o.require("magnitude", 1, 1); o.require("phase", 0, 0); o.require("joinMagphase", 0, 0);
    o.require("normalise", 0, 0); o.require("power", 0, 0); o.require("dBpsd", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  for (const ConfInstance *a : {acf, cep}) {              // src/dspcore/acf.cpp:46-55; usePower defaults to 0 with cepstrum = 1 (:91-102)
    const bool c = a == cep;
    OptReader o(*a);
    if (!wired(a, lvl(mag, "writer.dmLevel"))) return false;
    o.require("cepstrum", c ? 1 : 0, 0); o.require("usePower", c ? 0 : 1, c ? 0 : 1); o.require("inverse", 0, 0);
    o.require("cosLifterCepstrum", 0, 0); o.require("expBeforeAbs", 1, 1); o.require("symmetricData", 1, 1);
    o.require("acfCepsNormOutput", 1, 1); o.require("oldCompatCepstrum", 0, 0); o.require("absCepstrum", 0, 0);
    o.require("processArrayFields", 1, 1);
    o.str("nameAppend", "acf");                           // (cPitchACF names its outputs itself)
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lldcore/pitchACF.cpp:38-49, :96-103
    OptReader o(*pit);
    double mp = o.num("maxPitch", 500.0), vc = o.num("voicingCutoff", 0.55);
    if (vc > 1.0) vc = 1.0;
    if (vc < 0.0) vc = 0.0;
    if (mp < 0.0) mp = 0.0;
    p.f0_params["pitch_max"] = mp;
    p.f0_params["voicing_cutoff"] = vc;
    o.require("voiceProb", 1, 1); o.require("F0", 1, 0); o.require("F0raw", 0, 0); o.require("F0env", 0, 0); o.require("voiceQual", 0, 0);
    o.require("HNR", 0, 0); o.require("HNRdB", 0, 0); o.require("linHNR", 0, 0); o.require("processArrayFields", 0, 0);
    if (o.has("nameAppend") && !o.str("nameAppend", "").empty()) o.err = "[" + pit->name + ":cPitchACF] nameAppend is not expressible on the fused path (needs none)";
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/contourSmoother.cpp:33-36, src/core/windowProcessor.cpp:39
    OptReader o(*smo);
    if (!wired(smo, lvl(pit, "writer.dmLevel") + ";" + lvl(in, "writer.dmLevel"))) return false;
    const double w = o.num("smaWin", 3);
    if ((w < 3 || w > 9 || w != std::floor(w) || !((int)w & 1)) && o.err.empty())
      o.err = "[" + smo->name + ":cContourSmoother] smaWin = " + canonical_value(std::to_string(w)) + " is not expressible on the fused path (needs an odd number, 3 .. 9)";
    p.f0_params["sma_win"] = w;
    o.require("noZeroSma", 0, 0); o.require("noPostEOIprocessing", 0, 0);
    must_be(o, "nameAppend", "sma", "sma");
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  if (lvl(smo, "writer.dmLevel") != "lld") {
    err = "[" + smo->name + ":cContourSmoother] writer.dmLevel = '" + lvl(smo, "writer.dmLevel") + "', expected 'lld' (the level the shared output file's sinks read)";
    return false;
  }
  if (!conf_check_io(f, {"lld"}, err)) return false;
  p.preset = "prosody_acf";
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
  if (conf_fingerprint(f) == kProsodyAcfFingerprint) {     // the shipped file: the preset as it is
    p.f0_params.clear();
    p.describe = "the graph of prosodyAcf.conf (every processing component and option identical)";
    return true;
  }
  std::string what;
  for (const auto &kv : p.f0_params) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%s%s = %.9g", what.empty() ? "" : ", ", kv.first.c_str(), kv.second);
    what += buf;
  }
  p.describe = "the graph of prosodyAcf.conf with the file's own parameter values (" + what + ")";
  return true;
}

// ---- smilextract_hip --set chroma_fft -C file: config/chroma/chroma_fft.conf, possibly with other values of the options the chain takes
// as parameters (cTonespec nOctaves, firstNote, filterType, usePower, dbA; cChroma octaveSize, silThresh). Walked like prosodyAcf.conf
// above: every other option has the one value SMILEHIP_CHAIN_CHROMA_FFT implements or is refused by name. The file's one sink is a
// cCsvSink of values only (no header, time stamp or number column): what -O writes for this set. (Plain -C does not map the file.)
bool conf_to_chroma_fft(const ConfFile &f, ConfPlan &p, std::string &err) {
  p = ConfPlan();
  static const std::vector<std::string> types = {"cFramer", "cWindower", "cTransformFFT", "cFFTmagphase", "cTonespec", "cChroma"};
  std::map<std::string, const ConfInstance *> one;
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    if (std::find(types.begin(), types.end(), i.type) == types.end()) {
      err = "component [" + i.name + ":" + i.type + "] is not part of the graph of chroma_fft.conf";
      return false;
    }
    if (one.count(i.type)) { err = "more than one " + i.type + " ([" + i.name + "]): not the graph of chroma_fft.conf"; return false; }
    one[i.type] = &i;
  }
  for (const std::string &t : types)
    if (!one.count(t)) { err = "the graph has no " + t + ": not the graph of chroma_fft.conf"; return false; }
  auto lvl = [](const ConfInstance *i, const char *k) { const std::string *v = i->find(k); return v ? *v : std::string(); };
  auto wired = [&](const ConfInstance *i, const std::string &want) {
    if (lvl(i, "reader.dmLevel") == want) return true;
    err = "[" + i->name + ":" + i->type + "] reader.dmLevel = '" + lvl(i, "reader.dmLevel") + "', expected '" + want + "' (not the wiring of chroma_fft.conf)";
    return false;
  };
  auto must_be = [](OptReader &o, const char *key, const char *want, const char *dflt) {
    const std::string v = o.str(key, dflt);
    if (lower(v) != lower(want) && o.err.empty())
      o.err = "[" + o.ci.name + ":" + o.ci.type + "] " + key + " = " + v + " is not expressible on the fused path (needs " + want + ")";
  };
  const ConfInstance *fr = one["cFramer"], *win = one["cWindower"], *fft = one["cTransformFFT"], *mag = one["cFFTmagphase"],
                     *ts = one["cTonespec"], *ch = one["cChroma"];
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource" && !wired(fr, lvl(&i, "writer.dmLevel"))) return false;
  {                                                       // src/core/winToVecProcessor.cpp:51-83
    OptReader o(*fr);
    o.require("frameSize", 0.064, 0.025); o.require("frameStep", 0.01, 0.0);
    must_be(o, "frameMode", "fixed", "fixed"); must_be(o, "frameCenterSpecial", "left", "left");
    o.require("noPostEOIprocessing", 1, 1); o.require("frameSizeFrames", 0, 0); o.require("frameStepFrames", 0, 0);
    o.require("frameCenter", 0, 0); o.require("frameCenterFrames", 0, 0); o.require("allowLastFrameIncomplete", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/windower.cpp:36-49
    OptReader o(*win);
    if (!wired(win, lvl(fr, "writer.dmLevel"))) return false;
    const std::string wf = o.str("winFunc", "Han");
    if (win_func_of(wf) != SMILEHIP_WIN_GAUSS) o.err = "[" + win->name + ":cWindower] winFunc = " + wf + " is not expressible on the fused path (needs gauss)";
    o.require("gain", 1, 1); o.require("sigma", 0.4, 0.4); o.require("offset", 0, 0);
    o.require("fade", 0, 0); o.require("squareRoot", 0, 0); o.require("xshift", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/transformFft.cpp:34-35
    OptReader o(*fft);
    if (!wired(fft, lvl(win, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0); o.require("zeroPadSymmetric", 1, 1); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/fftmagphase.cpp:39-49
    OptReader o(*mag);
    if (!wired(mag, lvl(fft, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0); o.require("magnitude", 1, 1); o.require("phase", 0, 0); o.require("joinMagphase", 0, 0);
    o.require("normalise", 0, 0); o.require("power", 0, 0); o.require("dBpsd", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  int n_notes = 0;
  {                                                       // src/lld/tonespec.cpp:47-52, :89-117
    OptReader o(*ts);
    if (!wired(ts, lvl(mag, "writer.dmLevel"))) return false;
    const double no = o.num("nOctaves", 6), fn = o.num("firstNote", 55.0);
    if ((no < 1 || no > 10 || no != std::floor(no)) && o.err.empty())
      o.err = "[" + ts->name + ":cTonespec] nOctaves = " + canonical_value(std::to_string(no)) + " is not expressible on the fused path (needs 1 .. 10)";
    if (!(fn > 0.0) && o.err.empty())
      o.err = "[" + ts->name + ":cTonespec] firstNote = " + canonical_value(std::to_string(fn)) + " is not expressible on the fused path (needs a positive frequency)";
    n_notes = 12 * (int)no;
    const std::string ft = o.str("filterType", "gau");    // the spellings of :107-111; anything else leaves the component at gau
    static const std::pair<const char *, int> spell[] = {
        {"gau", 0}, {"Gau", 0}, {"gauss", 0}, {"Gauss", 0}, {"gaussian", 0}, {"Gaussian", 0}, {"tri", 1}, {"Tri", 1}, {"triangular", 1},
        {"Triangular", 1}, {"trp", 2}, {"TrP", 2}, {"Trp", 2}, {"triangular-powered", 2}, {"Triangular-Powered", 2}, {"rec", 3}, {"Rec", 3},
        {"rectangular", 3}, {"Rectangular", 3}};
    int type = -1;
    for (const auto &sp : spell)
      if (ft == sp.first) type = sp.second;
    if (type < 0 && o.err.empty())
      o.err = "[" + ts->name + ":cTonespec] filterType = " + ft + " is not expressible on the fused path (needs gau, tri, trp or rec)";
    p.f0_params["tonespec_n_octaves"] = no;
    p.f0_params["tonespec_first_note"] = (double)(float)fn;
    p.f0_params["tonespec_filter_type"] = type;
    p.f0_params["tonespec_use_power"] = o.num("usePower", 0) != 0.0;
    p.f0_params["tonespec_dba"] = o.num("dbA", 1) != 0.0;
    o.require("processArrayFields", 0, 1);
    o.str("nameAppend", "note");                          // (cChroma names its outputs itself: copyInputName = 0)
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lld/chroma.cpp:46-49, :67-75
    OptReader o(*ch);
    if (!wired(ch, lvl(ts, "writer.dmLevel"))) return false;
    const double os = o.num("octaveSize", 12), st = o.num("silThresh", 0.001);
    if ((os < 1 || os > 64 || os != std::floor(os) || (n_notes % (int)os)) && o.err.empty())
      o.err = "[" + ch->name + ":cChroma] octaveSize = " + canonical_value(std::to_string(os)) + " is not expressible on the fused path (needs 1 .. 64 and a divisor of the " +
              std::to_string(n_notes) + " notes)";
    p.f0_params["chroma_octave_size"] = os;
    p.f0_params["chroma_sil_thresh"] = (double)(float)st;
    o.require("processArrayFields", 0, 1);
    must_be(o, "nameAppend", "chroma", "chroma");
    o.require("copyInputName", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  if (!conf_check_io(f, {lvl(ch, "writer.dmLevel")}, err, true)) return false;
  p.preset = "chroma_fft";
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
  const std::map<std::string, double> shipped = {{"tonespec_n_octaves", 6}, {"tonespec_first_note", 55}, {"tonespec_filter_type", 0}, {"tonespec_use_power", 1},
                                                 {"tonespec_dba", 1}, {"chroma_octave_size", 12}, {"chroma_sil_thresh", (double)(float)0.001}};
  if (p.f0_params == shipped) {                           // the shipped file's values: the preset as it is
    p.f0_params.clear();
    p.describe = "the graph of chroma_fft.conf (every processing component and option identical)";
    return true;
  }
  std::string what;
  for (const auto &kv : p.f0_params) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%s%s = %.9g", what.empty() ? "" : ", ", kv.first.c_str(), kv.second);
    what += buf;
  }
  p.describe = "the graph of chroma_fft.conf with the file's own parameter values (" + what + ")";
  return true;
}

// ---- smilextract_hip --set spectrogram -C file: config/spectrum/spectrogram.conf with the file's own values. Walked like chroma_fft.conf
// above; the chain takes the framer's sizes, the window, zeroPadSymmetric and cFFTmagphase's form as parameters. (Plain -C does not
// map the file: tests/test_conf_plan.py fixes the set of files it maps.)
std::string spectrum_field_name(int flags) {
  if (flags & SMILEHIP_MAGPHASE_DBPSD) return "pcm_fftMag_dBsplPSD";
  const bool n = flags & SMILEHIP_MAGPHASE_NORMALISE, pw = flags & SMILEHIP_MAGPHASE_POWER;
  return pw ? (n ? "pcm_fftMag_PowSpecDens" : "pcm_fftMag_PowSpec") : (n ? "pcm_fftMag_SpecDens" : "pcm_fftMag");
}
bool conf_to_spectrogram(const ConfFile &f, ConfPlan &p, std::string &err) {
  p = ConfPlan();
  static const std::vector<std::string> types = {"cFramer", "cWindower", "cTransformFFT", "cFFTmagphase"};
  std::map<std::string, const ConfInstance *> one;
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    if (std::find(types.begin(), types.end(), i.type) == types.end()) {
      err = "component [" + i.name + ":" + i.type + "] is not part of the graph of spectrogram.conf";
      return false;
    }
    if (one.count(i.type)) { err = "more than one " + i.type + " ([" + i.name + "]): not the graph of spectrogram.conf"; return false; }
    one[i.type] = &i;
  }
  for (const std::string &t : types)
    if (!one.count(t)) { err = "the graph has no " + t + ": not the graph of spectrogram.conf"; return false; }
  auto lvl = [](const ConfInstance *i, const char *k) { const std::string *v = i->find(k); return v ? *v : std::string(); };
  auto wired = [&](const ConfInstance *i, const std::string &want) {
    if (lvl(i, "reader.dmLevel") == want) return true;
    err = "[" + i->name + ":" + i->type + "] reader.dmLevel = '" + lvl(i, "reader.dmLevel") + "', expected '" + want + "' (not the wiring of spectrogram.conf)";
    return false;
  };
  auto must_be = [](OptReader &o, const char *key, const char *want, const char *dflt) {
    const std::string v = o.str(key, dflt);
    if (lower(v) != lower(want) && o.err.empty())
      o.err = "[" + o.ci.name + ":" + o.ci.type + "] " + key + " = " + v + " is not expressible on the fused path (needs " + want + ")";
  };
  const ConfInstance *fr = one["cFramer"], *win = one["cWindower"], *fft = one["cTransformFFT"], *mag = one["cFFTmagphase"];
  smilehip_lld_config &c = p.cfg;
  smilehip_config_spectrogram(&c);
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource" && !wired(fr, lvl(&i, "writer.dmLevel"))) return false;
  {                                                       // src/core/winToVecProcessor.cpp:51-83
    OptReader o(*fr);
    c.frame_size_sec = o.num("frameSize", 0.025);
    c.frame_step_sec = o.num("frameStep", 0.0);
    if (c.frame_step_sec == 0.0) c.frame_step_sec = c.frame_size_sec;
    if (!(c.frame_size_sec > 0.0) && o.err.empty()) o.err = "[" + fr->name + ":cFramer] frameSize must be positive";
    must_be(o, "frameMode", "fixed", "fixed"); must_be(o, "frameCenterSpecial", "left", "left");
    o.require("noPostEOIprocessing", 1, 1); o.require("frameSizeFrames", 0, 0); o.require("frameStepFrames", 0, 0);
    o.require("frameCenter", 0, 0); o.require("frameCenterFrames", 0, 0); o.require("allowLastFrameIncomplete", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  std::string wf;
  {                                                       // src/dspcore/windower.cpp:36-49
    OptReader o(*win);
    if (!wired(win, lvl(fr, "writer.dmLevel"))) return false;
    wf = o.str("winFunc", "Han");
    c.win_func = win_func_of(wf);
    if (c.win_func < 0) o.err = "[" + win->name + ":cWindower] winFunc = " + wf + " is not expressible (Hann, Hamming, rectangular, Gauss, sine, triangle, Bartlett, Lanczos are)";
    c.win_gain = o.num("gain", 1.0);                      // (the plan's window table carries the gain)
    c.win_offset = o.num("offset", 0.0);
    c.win_sigma = o.num("sigma", 0.4);
    o.require("fade", 0, 0); o.require("squareRoot", 0, 0); o.require("xshift", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/transformFft.cpp:34-35
    OptReader o(*fft);
    if (!wired(fft, lvl(win, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0);
    c.zero_pad_symmetric = o.num("zeroPadSymmetric", 1) != 0.0;
    o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/fftmagphase.cpp:39-49, :72-97
    OptReader o(*mag);
    if (!wired(mag, lvl(fft, "writer.dmLevel"))) return false;
    o.require("inverse", 0, 0); o.require("magnitude", 1, 1); o.require("phase", 0, 0); o.require("joinMagphase", 0, 0);
    const bool normalise = o.num("normalise", 0) != 0.0, power = o.num("power", 0) != 0.0, db = o.num("dBpsd", 0) != 0.0;
    p.spectrum_flags = SMILEHIP_MAGPHASE_MAGNITUDE | (normalise || db ? SMILEHIP_MAGPHASE_NORMALISE : 0) | (power ? SMILEHIP_MAGPHASE_POWER : 0) |
                       (db ? SMILEHIP_MAGPHASE_DBPSD : 0);
    p.spectrum_dbp_norm = (float)o.num("dBpnorm", 90.302);
    p.spectrum_min_dbp = (float)o.num("mindBp", -102.0);
    o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  if (!conf_check_io(f, {lvl(mag, "writer.dmLevel")}, err)) return false;
  for (const ConfInstance &i : f.inst) {
    if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
    if (i.type == "cArffSink") {
      const std::string *fn = i.find("filename");
      if (fn && *fn != "?" && !fn->empty()) { err = "[" + i.name + ":cArffSink] is active (-arffoutput " + *fn + "): the ARFF sink is not built for the spectrogram set"; return false; }
    }
    if (i.type == "cHtkSink") { const std::string *pk = i.find("parmKind"); if (pk) p.parm_kind = atoi(pk->c_str()); }
  }
  p.lld_names = {spectrum_field_name(p.spectrum_flags)};
  std::ostringstream d;
  d << "spectrogram chain: " << c.frame_size_sec * 1e3 << " ms / " << c.frame_step_sec * 1e3 << " ms frames, winFunc " << wf << ", gain " << c.win_gain
    << ", zeroPadSymmetric " << c.zero_pad_symmetric << ", form " << p.lld_names[0];
  if (p.spectrum_flags & SMILEHIP_MAGPHASE_DBPSD) d << " (dBpnorm " << p.spectrum_dbp_norm << ", mindBp " << p.spectrum_min_dbp << " before the clamp to dBpnorm - 120)";
  p.describe = d.str();
  return true;
}

// ---- smilextract_hip --set chroma_filt -C file: config/chroma/chroma_filt.conf, possibly with other values of the options the chain takes
// as parameters (cTonefilt nNotes, firstNote, decayF0, decayFN, outputPeriod; cChroma octaveSize, silThresh). Walked like chroma_fft.conf
// above. An nNotes that is no multiple of octaveSize is refused: the binary then writes rows of zeros (cChroma logs an error per frame,
// chroma.cpp:113-115), which no chain here reproduces. (Plain -C does not map the file.)
bool conf_to_chroma_filt(const ConfFile &f, ConfPlan &p, std::string &err) {
  p = ConfPlan();
  static const std::vector<std::string> types = {"cTonefilt", "cChroma"};
  std::map<std::string, const ConfInstance *> one;
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    if (std::find(types.begin(), types.end(), i.type) == types.end()) {
      err = "component [" + i.name + ":" + i.type + "] is not part of the graph of chroma_filt.conf";
      return false;
    }
    if (one.count(i.type)) { err = "more than one " + i.type + " ([" + i.name + "]): not the graph of chroma_filt.conf"; return false; }
    one[i.type] = &i;
  }
  for (const std::string &t : types)
    if (!one.count(t)) { err = "the graph has no " + t + ": not the graph of chroma_filt.conf"; return false; }
  auto lvl = [](const ConfInstance *i, const char *k) { const std::string *v = i->find(k); return v ? *v : std::string(); };
  auto wired = [&](const ConfInstance *i, const std::string &want) {
    if (lvl(i, "reader.dmLevel") == want) return true;
    err = "[" + i->name + ":" + i->type + "] reader.dmLevel = '" + lvl(i, "reader.dmLevel") + "', expected '" + want + "' (not the wiring of chroma_filt.conf)";
    return false;
  };
  auto must_be = [](OptReader &o, const char *key, const char *want, const char *dflt) {
    const std::string v = o.str(key, dflt);
    if (lower(v) != lower(want) && o.err.empty())
      o.err = "[" + o.ci.name + ":" + o.ci.type + "] " + key + " = " + v + " is not expressible on the fused path (needs " + want + ")";
  };
  const ConfInstance *tf = one["cTonefilt"], *ch = one["cChroma"];
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource") {
      if (!wired(tf, lvl(&i, "writer.dmLevel"))) return false;
      const std::string *mm = i.find("monoMixdown");        // (waveSource.cpp: the default is 1; the chain filters ONE channel)
      if (mm && canonical_value(*mm) != "1") { err = "[" + i.name + ":cWaveSource] monoMixdown = " + *mm + " is not expressible on the fused path (needs 1)"; return false; }
    }
  int n_notes = 0;
  {                                                       // src/lld/tonefilt.cpp:33-41, :65-98
    OptReader o(*tf);
    double nn = o.num("nNotes", 48), fn = o.num("firstNote", 55.0), d0 = o.num("decayF0", 0.9995), dn = o.num("decayFN", 0.998), op = o.num("outputPeriod", 0.1);
    if ((nn < 1 || nn > 120 || nn != std::floor(nn)) && o.err.empty())
      o.err = "[" + tf->name + ":cTonefilt] nNotes = " + canonical_value(std::to_string(nn)) + " is not expressible on the fused path (needs 1 .. 120)";
    if (!(fn > 0.0) && o.err.empty())
      o.err = "[" + tf->name + ":cTonefilt] firstNote = " + canonical_value(std::to_string(fn)) + " is not expressible on the fused path (needs a positive frequency)";
    if (!(op > 0.0) && o.err.empty())
      o.err = "[" + tf->name + ":cTonefilt] outputPeriod = " + canonical_value(std::to_string(op)) + " is not expressible on the fused path (needs a positive period)";
    n_notes = (int)nn;
    p.f0_params["tonefilt_n_notes"] = nn;
    p.f0_params["tonefilt_first_note"] = fn;
    p.f0_params["tonefilt_decay_f0"] = d0;                // (clamped by the chain as the component clamps them)
    p.f0_params["tonefilt_decay_fn"] = dn;
    p.f0_params["tonefilt_output_period"] = op;
    o.str("nameAppend", "tonefilt");                      // (cChroma names its outputs itself: copyInputName = 0)
    o.num("copyInputName", 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lld/chroma.cpp:46-49, :67-75
    OptReader o(*ch);
    if (!wired(ch, lvl(tf, "writer.dmLevel"))) return false;
    const double os = o.num("octaveSize", 12), st = o.num("silThresh", 0.001);
    if ((os < 1 || os > 64 || os != std::floor(os) || (n_notes % (int)os)) && o.err.empty())
      o.err = "[" + ch->name + ":cChroma] octaveSize = " + canonical_value(std::to_string(os)) + " is not expressible on the fused path (needs 1 .. 64 and a divisor of the " +
              std::to_string(n_notes) + " notes of nNotes)";
    p.f0_params["chroma_octave_size"] = os;
    p.f0_params["chroma_sil_thresh"] = (double)(float)st;
    o.num("processArrayFields", 1);                       // (either value: cTonefilt writes ONE array field of nNotes elements per input channel)
    must_be(o, "nameAppend", "chroma", "chroma");
    o.require("copyInputName", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  if (!conf_check_io(f, {lvl(ch, "writer.dmLevel")}, err, true)) return false;
  p.preset = "chroma_filt";
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
  const std::map<std::string, double> shipped = {{"tonefilt_n_notes", 72}, {"tonefilt_first_note", 55}, {"tonefilt_decay_f0", 0.9999}, {"tonefilt_decay_fn", 0.999},
                                                 {"tonefilt_output_period", 0.01}, {"chroma_octave_size", 12}, {"chroma_sil_thresh", (double)(float)0.001}};
  if (p.f0_params == shipped) {                           // the shipped file's values: the preset as it is
    p.f0_params.clear();
    p.describe = "the graph of chroma_filt.conf (every processing component and option identical)";
    return true;
  }
  std::string what;
  for (const auto &kv : p.f0_params) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%s%s = %.9g", what.empty() ? "" : ", ", kv.first.c_str(), kv.second);
    what += buf;
  }
  p.describe = "the graph of chroma_filt.conf with the file's own parameter values (" + what + ")";
  return true;
}

// ---- smilextract_hip --set emobase -C file: config/emobase/emobase.conf, levels lld and lld_de, possibly with other values of the
// options the chain takes as parameters (cPitchACF maxPitch, voicingCutoff; cContourSmoother smaWin; cLpc p). Walked like
// prosodyAcf.conf above: every other option has the one value SMILEHIP_CHAIN_EMOBASE implements or is refused by name. The
// cFunctionals instance behind the two levels is passed over (its level is not built: a sink on it is refused by conf_check_io).
// fingerprint of the reference's own file with its includes and every command-line option at its default (--fingerprint prints it)
static const uint64_t kEmobaseFingerprint = 0xbb4eb6d6855829baull;
bool conf_to_emobase(const ConfFile &f, ConfPlan &p, std::string &err) {
  p = ConfPlan();
  const char *graph = "not the graph of emobase.conf";
  static const std::map<std::string, int> count_of = {{"cFramer", 2}, {"cWindower", 2}, {"cTransformFFT", 2}, {"cFFTmagphase", 2}, {"cAcf", 2},
      {"cPitchACF", 1}, {"cVectorPreemphasis", 1}, {"cMelspec", 1}, {"cMfcc", 1}, {"cLpc", 1}, {"cLsp", 1}, {"cMZcr", 1}, {"cIntensity", 1},
      {"cContourSmoother", 1}, {"cDeltaRegression", 1}, {"cFunctionals", 1}};
  std::map<std::string, std::vector<const ConfInstance *>> by_type;
  for (const ConfInstance &i : f.inst) {
    if (is_io_type(i.type)) continue;
    if (!count_of.count(i.type)) { err = "component [" + i.name + ":" + i.type + "] is not part of the graph of emobase.conf"; return false; }
    by_type[i.type].push_back(&i);
  }
  for (const auto &kv : count_of) {
    const size_t n = by_type.count(kv.first) ? by_type[kv.first].size() : 0;
    if (kv.first == "cFunctionals" ? n > 1 : n != (size_t)kv.second) {
      err = "the graph has " + std::to_string(n) + " " + kv.first + " instance(s), emobase.conf has " + std::to_string(kv.second) + ": " + graph;
      return false;
    }
  }
  auto lvl = [](const ConfInstance *i, const char *k) { const std::string *v = i->find(k); return v ? *v : std::string(); };
  auto wired = [&](const ConfInstance *i, const std::string &want) {
    if (lvl(i, "reader.dmLevel") == want) return true;
    err = "[" + i->name + ":" + i->type + "] reader.dmLevel = '" + lvl(i, "reader.dmLevel") + "', expected '" + want + "' (not the wiring of emobase.conf)";
    return false;
  };
  auto must_be = [](OptReader &o, const char *key, const char *want, const char *dflt) {
    const std::string v = o.str(key, dflt);
    if (lower(v) != lower(want) && o.err.empty())
      o.err = "[" + o.ci.name + ":" + o.ci.type + "] " + key + " = " + v + " is not expressible on the fused path (needs " + want + ")";
  };
  auto reads = [&](const char *type, const std::string &level) -> const ConfInstance * {   // the instance of `type` that reads `level`
    for (const ConfInstance *i : by_type[type]) if (lvl(i, "reader.dmLevel") == level) return i;
    return nullptr;
  };
  auto missing = [&](const char *type, const std::string &level) {
    err = std::string("no ") + type + " reads level '" + level + "' (not the wiring of emobase.conf)";
    return false;
  };
  // the two framers on `wave`, told apart by their frame size
  const ConfInstance *fr25 = nullptr, *fr40 = nullptr;
  for (const ConfInstance *fr : by_type["cFramer"]) {    // src/core/winToVecProcessor.cpp:51-83
    OptReader o(*fr);
    if (!wired(fr, "wave")) return false;
    const double fsz = o.num("frameSize", 0.025);
    if (fsz == 0.025 && !fr25) fr25 = fr;
    else if (fsz == 0.04 && !fr40) fr40 = fr;
    else if (o.err.empty())
      o.err = "[" + fr->name + ":cFramer] frameSize = " + canonical_value(std::to_string(fsz)) + " is not expressible on the fused path (needs 0.025 and 0.04, one framer each)";
    o.require("frameStep", 0.01, 0.0);
    must_be(o, "frameMode", "fixed", "fixed"); must_be(o, "frameCenterSpecial", "left", "left");
    o.require("noPostEOIprocessing", 1, 1); o.require("frameSizeFrames", 0, 0); o.require("frameStepFrames", 0, 0);
    o.require("frameCenter", 0, 0); o.require("frameCenterFrames", 0, 0); o.require("allowLastFrameIncomplete", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  const std::string frames25 = lvl(fr25, "writer.dmLevel"), frames40 = lvl(fr40, "writer.dmLevel");
  auto window_chain = [&](const std::string &in, const ConfInstance *&mag_out) {   // cWindower -> cTransformFFT -> cFFTmagphase behind level `in`
    const ConfInstance *win = reads("cWindower", in);
    if (!win) return missing("cWindower", in);
    {                                                     // src/dspcore/windower.cpp:36-49
      OptReader o(*win);
      const std::string wf = o.str("winFunc", "Han");
      if (win_func_of(wf) != SMILEHIP_WIN_HAMM) o.err = "[" + win->name + ":cWindower] winFunc = " + wf + " is not expressible on the fused path (needs ham)";
      o.require("gain", 1, 1); o.require("offset", 0, 0); o.require("fade", 0, 0); o.require("squareRoot", 0, 0); o.require("xshift", 0, 0);
      o.require("processArrayFields", 1, 1);
      o.num("sigma", 0.4); o.num("alpha", 0.16); o.num("alpha0", 0); o.num("alpha1", 0); o.num("alpha2", 0); o.num("alpha3", 0);   // (not read by ham)
      if (!o.finish(kBenign)) { err = o.err; return false; }
    }
    const ConfInstance *fft = reads("cTransformFFT", lvl(win, "writer.dmLevel"));
    if (!fft) return missing("cTransformFFT", lvl(win, "writer.dmLevel"));
    {                                                     // src/dspcore/transformFft.cpp:34-35
      OptReader o(*fft);
      o.require("inverse", 0, 0); o.require("zeroPadSymmetric", 0, 1); o.require("processArrayFields", 1, 1);
      if (!o.finish(kBenign)) { err = o.err; return false; }
    }
    const ConfInstance *mag = reads("cFFTmagphase", lvl(fft, "writer.dmLevel"));
    if (!mag) return missing("cFFTmagphase", lvl(fft, "writer.dmLevel"));
    {                                                     // src/dspcore/fftmagphase.cpp:39-49
      OptReader o(*mag);
      o.require("inverse", 0, 0); o.require("magnitude", 1, 1); o.require("phase", 0, 0); o.require("joinMagphase", 0, 0);
      o.require("normalise", 0, 0); o.require("power", 0, 0); o.require("dBpsd", 0, 0); o.require("processArrayFields", 1, 1);
      if (!o.finish(kBenign)) { err = o.err; return false; }
    }
    mag_out = mag;
    return true;
  };
  // ---- 40 ms: window, transform, magnitudes, two cAcf, cPitchACF
  const ConfInstance *mag40 = nullptr;
  if (!window_chain(frames40, mag40)) return false;
  const ConfInstance *pit = by_type["cPitchACF"][0];
  const std::vector<std::string> pin = split_levels(lvl(pit, "reader.dmLevel"));
  const ConfInstance *acf = nullptr, *cep = nullptr;
  if (pin.size() == 2)
    for (const ConfInstance *a : by_type["cAcf"]) {
      if (lvl(a, "writer.dmLevel") == pin[0] && !acf) acf = a;
      else if (lvl(a, "writer.dmLevel") == pin[1] && !cep) cep = a;
    }
  if (!acf || !cep) {
    err = "[" + pit->name + ":cPitchACF] reader.dmLevel = '" + lvl(pit, "reader.dmLevel") + "', expected the levels of the two cAcf instances, ACF first (not the wiring of emobase.conf)";
    return false;
  }
  for (const ConfInstance *a : {acf, cep}) {              // src/dspcore/acf.cpp:46-55, :91-108
    const bool c = a == cep;
    OptReader o(*a);
    if (!wired(a, lvl(mag40, "writer.dmLevel"))) return false;
    o.require("cepstrum", c ? 1 : 0, 0); o.require("usePower", 1, c ? 0 : 1); o.require("inverse", 0, 0);
    o.require("cosLifterCepstrum", 0, 0); o.require("expBeforeAbs", 1, 1); o.require("symmetricData", 1, 1);
    o.require("oldCompatCepstrum", c ? 1 : 0, 0);
    if (c) { o.num("acfCepsNormOutput", 0); o.num("absCepstrum", 1); }   // (oldCompatCepstrum forces absCepstrum = 1 and acfCepsNormOutput = 0, acf.cpp:103-108)
    else { o.require("acfCepsNormOutput", 0, 1); o.num("absCepstrum", 0); }   // (absCepstrum: not read without cepstrum)
    o.require("processArrayFields", 1, 1);
    o.str("nameAppend", "acf");                           // (cPitchACF names its outputs itself)
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lldcore/pitchACF.cpp:38-49, :96-103
    OptReader o(*pit);
    double mp = o.num("maxPitch", 500.0), vc = o.num("voicingCutoff", 0.55);
    if (vc > 1.0) vc = 1.0;
    if (vc < 0.0) vc = 0.0;
    if (mp < 0.0) mp = 0.0;
    p.f0_params["pitch_max"] = mp;
    p.f0_params["voicing_cutoff"] = vc;
    o.require("voiceProb", 1, 1); o.require("F0", 1, 0); o.require("F0raw", 0, 0); o.require("F0env", 1, 0); o.require("voiceQual", 0, 0);
    o.require("HNR", 0, 0); o.require("HNRdB", 0, 0); o.require("linHNR", 0, 0); o.require("processArrayFields", 0, 0);
    if (o.has("nameAppend") && !o.str("nameAppend", "").empty()) o.err = "[" + pit->name + ":cPitchACF] nameAppend is not expressible on the fused path (needs none)";
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  // ---- 25 ms: cIntensity and cMZcr on the frames, cVectorPreemphasis, then cLpc -> cLsp and window .. cMelspec -> cMfcc
  const ConfInstance *in = by_type["cIntensity"][0], *zc = by_type["cMZcr"][0], *pe = by_type["cVectorPreemphasis"][0], *lpc = by_type["cLpc"][0],
                     *lsp = by_type["cLsp"][0], *mel = by_type["cMelspec"][0], *mfcc = by_type["cMfcc"][0], *smo = by_type["cContourSmoother"][0],
                     *del = by_type["cDeltaRegression"][0];
  {                                                       // src/lldcore/intensity.cpp:36-38
    OptReader o(*in);
    if (!wired(in, frames25)) return false;
    o.require("intensity", 1, 1); o.require("loudness", 1, 0); o.require("processArrayFields", 1, 1);
    if (o.has("nameAppend") && !o.str("nameAppend", "").empty()) o.err = "[" + in->name + ":cIntensity] nameAppend is not expressible on the fused path (needs none)";
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lldcore/mzcr.cpp:36-42
    OptReader o(*zc);
    if (!wired(zc, frames25)) return false;
    o.require("zcr", 1, 1); o.require("mcr", 0, 1); o.require("amax", 0, 1); o.require("maxmin", 0, 1); o.require("dc", 0, 0); o.require("processArrayFields", 1, 1);
    if (o.has("nameAppend") && !o.str("nameAppend", "").empty()) o.err = "[" + zc->name + ":cMZcr] nameAppend is not expressible on the fused path (needs none)";
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/vectorPreemphasis.cpp:38-41
    OptReader o(*pe);
    if (!wired(pe, frames25)) return false;
    const double k = o.num("k", 0.97);
    if ((float)k != 0.97f && o.err.empty()) o.err = "[" + pe->name + ":cVectorPreemphasis] k = " + canonical_value(std::to_string(k)) + " is not expressible on the fused path (needs 0.97)";
    o.require("de", 0, 0); o.require("f", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  const std::string framespe = lvl(pe, "writer.dmLevel");
  {                                                       // src/lld/lpc.cpp:45-58
    OptReader o(*lpc);
    if (!wired(lpc, framespe)) return false;
    must_be(o, "method", "acf", "acf");
    const double order = o.num("p", 8);
    if ((order < 2 || order > 16 || order != std::floor(order) || ((int)order & 1)) && o.err.empty())
      o.err = "[" + lpc->name + ":cLpc] p = " + canonical_value(std::to_string(order)) + " is not expressible on the fused path (needs an even number, 2 .. 16)";
    p.f0_params["lpc_order"] = order;
    o.require("saveLPCoeff", 1, 1); o.require("lpGain", 0, 0); o.require("saveRefCoeff", 0, 0); o.require("residual", 0, 0);
    o.require("residualGainScale", 0, 0); o.require("forwardFilter", 0, 0); o.require("lpSpectrum", 0, 0); o.require("forwardLPspec", 1, 1);
    o.require("processArrayFields", 1, 1);
    o.num("lpSpecDeltaF", 10); o.num("lpSpecBins", 100);  // (read with lpSpectrum alone)
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lld/lsp.cpp:43-47
    OptReader o(*lsp);
    if (!wired(lsp, lvl(lpc, "writer.dmLevel"))) return false;
    o.require("processArrayFields", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  const ConfInstance *mag25 = nullptr;
  if (!window_chain(framespe, mag25)) return false;
  {                                                       // src/lldcore/melspec.cpp:40-53
    OptReader o(*mel);
    if (!wired(mel, lvl(mag25, "writer.dmLevel"))) return false;
    o.require("nBands", 26, 26); o.require("lofreq", 0, 20); o.require("hifreq", 8000, 8000); o.require("usePower", 1, 0);
    o.require("htkcompatible", 1, 1); o.require("inverse", 0, 0); o.require("showFbank", 0, 0); o.require("processArrayFields", 1, 1);
    must_be(o, "specScale", "mel", "mel");
    o.num("bwMethod", 0); o.num("logScaleBase", 2); o.num("firstNote", 27.5); o.num("halfBwTarg", 0);   // (not read on the mel scale)
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/lldcore/mfcc.cpp:40-48
    OptReader o(*mfcc);
    if (!wired(mfcc, lvl(mel, "writer.dmLevel"))) return false;
    o.require("firstMfcc", 1, 1); o.require("lastMfcc", 12, 12); o.require("cepLifter", 22, 22); o.require("htkcompatible", 1, 1);
    o.require("nMfcc", 12, 12); o.require("melfloor", 1e-8, 1e-8); o.require("doLog", 1, 1); o.require("inverse", 0, 0);
    o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  {                                                       // src/dspcore/contourSmoother.cpp:33-36, src/core/windowProcessor.cpp:39
    OptReader o(*smo);
    if (!wired(smo, lvl(in, "writer.dmLevel") + ";" + lvl(mfcc, "writer.dmLevel") + ";" + lvl(lsp, "writer.dmLevel") + ";" + lvl(zc, "writer.dmLevel") + ";" +
                        lvl(pit, "writer.dmLevel")))
      return false;
    const double w = o.num("smaWin", 3);
    if ((w < 3 || w > 9 || w != std::floor(w) || !((int)w & 1)) && o.err.empty())
      o.err = "[" + smo->name + ":cContourSmoother] smaWin = " + canonical_value(std::to_string(w)) + " is not expressible on the fused path (needs an odd number, 3 .. 9)";
    p.f0_params["sma_win"] = w;
    o.require("noZeroSma", 0, 0); o.require("noPostEOIprocessing", 0, 0);
    must_be(o, "nameAppend", "sma", "sma");
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  if (lvl(smo, "writer.dmLevel") != "lld") {
    err = "[" + smo->name + ":cContourSmoother] writer.dmLevel = '" + lvl(smo, "writer.dmLevel") + "', expected 'lld' (the level the shared output file's sinks read)";
    return false;
  }
  {                                                       // src/dspcore/deltaRegression.cpp:38-44
    OptReader o(*del);
    if (!wired(del, "lld")) return false;
    o.require("deltawin", 2, 2); o.require("absOutput", 0, 0); o.require("halfWaveRect", 0, 0); o.require("onlyInSegments", 0, 0);
    o.require("zeroSegBound", 1, 1); o.require("relativeDelta", 0, 0); o.require("noPostEOIprocessing", 0, 0);
    must_be(o, "nameAppend", "de", "de");
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  if (lvl(del, "writer.dmLevel") != "lld_de") {
    err = "[" + del->name + ":cDeltaRegression] writer.dmLevel = '" + lvl(del, "writer.dmLevel") + "', expected 'lld_de' (the level the shared output file's sinks read)";
    return false;
  }
  for (const ConfInstance &i : f.inst) {                   // an active sink on the functionals level: said by its name
    const std::string *fn = i.find("filename");
    const bool sink = i.type.size() > 4 && i.type.compare(i.type.size() - 4, 4, "Sink") == 0;
    if (sink && fn && *fn != "?" && lvl(&i, "reader.dmLevel") == "func") {
      err = "[" + i.name + ":" + i.type + "] is active (filename = " + *fn + "): the functionals level of emobase.conf is not built yet (the levels lld and lld_de are: -lldcsvoutput, -lldhtkoutput)";
      return false;
    }
  }
  if (!conf_check_io(f, {"lld", "lld_de"}, err)) return false;
  p.preset = "emobase";
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
  if (conf_fingerprint(f) == kEmobaseFingerprint) {        // the shipped file: the preset as it is
    p.f0_params.clear();
    p.describe = "the graph of emobase.conf, levels lld and lld_de (every processing component and option identical)";
    return true;
  }
  std::string what;
  for (const auto &kv : p.f0_params) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%s%s = %.9g", what.empty() ? "" : ", ", kv.first.c_str(), kv.second);
    what += buf;
  }
  p.describe = "the graph of emobase.conf, levels lld and lld_de, with the file's own parameter values (" + what + ")";
  return true;
}

static bool conf_to_plan_inner(const ConfFile &f, ConfPlan &p, std::string &err, bool audspec_set);
static bool conf_to_plan_any(const ConfFile &f, ConfPlan &p, std::string &err, bool audspec_set) {
  const bool ok = conf_to_plan_inner(f, p, err, audspec_set);
  if (ok && p.wave_file.empty())                         // (the big sets return before the cepstral walk that records it)
    for (const ConfInstance &i : f.inst)
      if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
  return ok;
}
bool conf_to_plan(const ConfFile &f, ConfPlan &p, std::string &err) { return conf_to_plan_any(f, p, err, false); }
// smilextract_hip --set audspec | audspec_compat -C file: the same walk with the auditory-spectrum cut of cPlp admitted (plain -C keeps
// to the files it has always mapped and names this route); any other graph is refused here
bool conf_to_audspec(const ConfFile &f, ConfPlan &p, std::string &err) {
  if (!conf_to_plan_any(f, p, err, true)) return false;
  if (!p.audspec) { err = "the file is not an auditory-spectrum chain (a cPlp with doIDFT = 0, doLP = 0, doLpToCeps = 0): use plain -C for it"; return false; }
  return true;
}
static bool conf_to_plan_inner(const ConfFile &f, ConfPlan &p, std::string &err, bool audspec_set) {
  p = ConfPlan();
  const uint64_t fp = conf_fingerprint(f);
  for (const KnownSet &k : kKnownSets)
    if (k.fingerprint == fp && fp != 0) {
      if (!conf_check_io(f, {"lld", "lld_de", "func"}, err)) return false;   // the shared output file's levels
      p.preset = k.set;
      p.describe = std::string("the graph of ") + k.file + " (every processing component and option identical)";
      return true;
    }
  // the same graph with other values of the options the kernels take as parameters (the F0 group's pitch range, harmonics,
  // compression, voicing cutoff, Viterbi buffer, jitter search range / threshold rule, energy gate)
  const uint64_t fpm = conf_fingerprint_masked(f);
  for (const KnownSet &k : kKnownSets)
    if (k.masked != 0 && k.masked == fpm) {
      if (!conf_check_io(f, {"lld", "lld_de", "func"}, err)) return false;
      p.preset = k.set;
      std::string what;
      for (const ConfInstance &i : f.inst)
        for (const auto &kv : i.opts) {
          const char *field = conf_is_f0_param(i, kv.first);
          if (!field) continue;
          char *end = nullptr;
          const double v = strtod(kv.second.c_str(), &end);
          if (end == kv.second.c_str()) { err = "[" + i.name + ":" + i.type + "] " + kv.first + " = " + kv.second + " is not a number"; return false; }
          p.f0_params[field] = v;
          what += (what.empty() ? "" : ", ") + kv.first + " = " + canonical_value(kv.second);
        }
      p.describe = std::string("the graph of ") + k.file + " with the file's own parameter values (" + what + ")";
      return true;
    }
  // the ComParE graphs with a lower lastMfcc and / or functional families removed: outputs of the shipped graph left out
  const uint64_t fpm2 = conf_fingerprint_masked2(f);
  for (const KnownSet &k : kKnownSets)
    if (k.masked2 != 0 && k.masked2 == fpm2) {
      if (!conf_check_io(f, {"lld", "lld_de", "func"}, err)) return false;
      p.preset = k.set;
      std::string what;
      for (const ConfInstance &i : f.inst)
        for (const auto &kv : i.opts) {
          if (const char *field = conf_is_f0_param(i, kv.first)) {
            char *end = nullptr;
            const double v = strtod(kv.second.c_str(), &end);
            if (end == kv.second.c_str()) { err = "[" + i.name + ":" + i.type + "] " + kv.first + " = " + kv.second + " is not a number"; return false; }
            p.f0_params[field] = v;
          } else if (i.type == "cMfcc" && kv.first == "lastMfcc") {
            p.last_mfcc = atoi(kv.second.c_str());
            if (p.last_mfcc < 1 || p.last_mfcc > 14) { err = "[" + i.name + ":cMfcc] lastMfcc = " + kv.second + ": the fused ComParE chain computes MFCC 1 .. 14 (a lower lastMfcc drops columns; a higher one is not built)"; return false; }
            what += (what.empty() ? "" : ", ") + std::string("lastMfcc = ") + kv.second;
          } else if (i.type == "cFunctionals" && kv.first == "functionalsEnabled") {
            const size_t at = i.name.find("functionals");
            const std::string inst = at == std::string::npos ? i.name : i.name.substr(at + 11);
            std::vector<std::string> fams;
            std::string tok;
            for (char ch : kv.second + ";") {
              if (ch == ';') { if (!tok.empty()) fams.push_back(tok); tok.clear(); }
              else if (!isspace((unsigned char)ch)) tok += ch;
            }
            p.func_enabled[inst] = fams;
            what += (what.empty() ? "" : ", ") + i.name + ".functionalsEnabled = " + kv.second;
          }
        }
      p.describe = std::string("the graph of ") + k.file + " with outputs left out (" + what + ")";
      return true;
    }
  // ---- a cepstral chain: framer -> [pre-emphasis] -> window -> FFT -> magnitude -> mel -> MFCC | PLP, optional log energy,
  // optional mean normalisation, delta regression, concatenation
  std::map<std::string, std::vector<const ConfInstance *>> by_type;
  const ConfInstance *htk_sink = nullptr, *any_sink = nullptr;
  for (const ConfInstance &i : f.inst) {
    if (i.type == "cHtkSink" && !htk_sink) htk_sink = &i;
    if (i.type.size() > 4 && i.type.compare(i.type.size() - 4, 4, "Sink") == 0 && !any_sink) any_sink = &i;
    if (!is_io_type(i.type)) by_type[i.type].push_back(&i);
  }
  static const std::set<std::string> chain_types = {"cFramer", "cVectorPreemphasis", "cWindower", "cTransformFFT", "cFFTmagphase", "cMelspec",
                                                    "cMfcc", "cPlp", "cEnergy", "cFullinputMean", "cDeltaRegression", "cVectorConcat"};
  for (const auto &kv : by_type)
    if (!chain_types.count(kv.first)) {
      err = "component [" + kv.second[0]->name + ":" + kv.first + "] is not part of a graph the fused path knows (the cepstral chains of "
            "config/mfcc and config/plp with any option values; IS09_emotion, ComParE_2016, IS13_ComParE, eGeMAPSv02 as shipped)";
      return false;
    }
  auto one = [&](const char *t, bool required) -> const ConfInstance * {
    auto it = by_type.find(t);
    if (it == by_type.end()) {
      if (required) err = std::string("the graph has no ") + t;
      return nullptr;
    }
    if (it->second.size() != 1) { err = std::string("more than one ") + t + " (one cepstral chain per file is expressible)"; return nullptr; }
    return it->second[0];
  };
  const ConfInstance *fr = one("cFramer", true), *win = one("cWindower", true), *fft = one("cTransformFFT", true),
                     *mag = one("cFFTmagphase", true), *mel = one("cMelspec", true);
  if (!err.empty()) return false;
  const ConfInstance *pe = one("cVectorPreemphasis", false), *en = one("cEnergy", false);
  one("cFullinputMean", false);
  if (!err.empty()) return false;
  const ConfInstance *mf = one("cMfcc", false), *pl = one("cPlp", false);
  if (!err.empty()) return false;
  if ((mf != nullptr) == (pl != nullptr)) { err = "the graph needs exactly one of cMfcc / cPlp"; return false; }
  smilehip_lld_config &c = p.cfg;
  smilehip_config_mfcc12_0_d_a(&c);
  p.plp = pl != nullptr;
  if (p.plp) smilehip_config_plp_0_d_a(&c);
  auto lvl = [](const ConfInstance *i, const char *k) { const std::string *v = i->find(k); return v ? *v : std::string(); };
  auto wired = [&](const ConfInstance *i, const std::string &want) {
    if (lvl(i, "reader.dmLevel") == want) return true;
    err = "[" + i->name + ":" + i->type + "] reads '" + lvl(i, "reader.dmLevel") + "', expected '" + want + "' (not the cepstral chain's wiring)";
    return false;
  };
  // cFramer (src/core/winToVecProcessor.cpp:51-83)
  {
    OptReader o(*fr);
    if (!wired(fr, "wave")) return false;
    c.frame_size_sec = o.num("frameSize", 0.025);
    c.frame_step_sec = o.num("frameStep", 0.0);
    if (c.frame_step_sec == 0.0) c.frame_step_sec = c.frame_size_sec;
    if (lower(o.str("frameMode", "fixed")) != "fixed") o.err = "[" + fr->name + ":cFramer] only frameMode = fixed is expressible";
    if (lower(o.str("frameCenterSpecial", "left")) != "left") o.err = "[" + fr->name + ":cFramer] only frameCenterSpecial = left is expressible";
    o.require("noPostEOIprocessing", 1, 1);
    o.require("frameSizeFrames", 0, 0); o.require("frameStepFrames", 0, 0); o.require("frameCenter", 0, 0);
    o.require("frameCenterFrames", 0, 0); o.require("allowLastFrameIncomplete", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
  }
  std::string level = lvl(fr, "writer.dmLevel");
  const std::string frames_level = level;
  for (const ConfInstance *st : {pe, win, fft, mag, mel})
    if (st) p.stage_levels.push_back(lvl(st, "writer.dmLevel"));
  for (const ConfInstance &i : f.inst)
    if (i.type == "cWaveSource") { const std::string *fn = i.find("filename"); if (fn) p.wave_file = *fn; }
  c.preemph = 0;
  if (pe) {                                             // src/dspcore/vectorPreemphasis.cpp:33-35
    OptReader o(*pe);
    if (!wired(pe, level)) return false;
    c.preemph = 1;
    c.preemph_k = (float)o.num("k", 0.97);
    c.preemph_de = (int)o.num("de", 0);
    o.require("f", 0, 0);
    if (!o.finish(kBenign)) { err = o.err; return false; }
    level = lvl(pe, "writer.dmLevel");
  }
  {                                                     // src/dspcore/windower.cpp:36-49
    OptReader o(*win);
    if (!wired(win, level)) return false;
    const std::string wf = o.str("winFunc", "Han");
    c.win_func = win_func_of(wf);
    if (c.win_func < 0) o.err = "[" + win->name + ":cWindower] winFunc = " + wf + " is not expressible (Hann, Hamming, rectangular, Gauss, sine, triangle, Bartlett, Lanczos are)";
    c.win_gain = o.num("gain", 1.0);
    c.win_offset = o.num("offset", 0.0);
    c.win_sigma = o.num("sigma", 0.4);
    o.require("fade", 0, 0); o.require("squareRoot", 0, 0); o.require("xshift", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
    level = lvl(win, "writer.dmLevel");
  }
  {                                                     // src/dspcore/transformFft.cpp:34-35
    OptReader o(*fft);
    if (!wired(fft, level)) return false;
    o.require("inverse", 0, 0);
    c.zero_pad_symmetric = (int)o.num("zeroPadSymmetric", 1);
    o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
    level = lvl(fft, "writer.dmLevel");
  }
  {                                                     // src/dspcore/fftmagphase.cpp:39-49
    OptReader o(*mag);
    if (!wired(mag, level)) return false;
    o.require("inverse", 0, 0); o.require("magnitude", 1, 1); o.require("phase", 0, 0); o.require("joinMagphase", 0, 0);
    o.require("normalise", 0, 0); o.require("power", 0, 0); o.require("dBpsd", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
    level = lvl(mag, "writer.dmLevel");
  }
  {                                                     // src/lldcore/melspec.cpp:32-44
    OptReader o(*mel);
    if (!wired(mel, level)) return false;
    c.n_bands = (int)o.num("nBands", 26);
    c.lofreq = (float)o.num("lofreq", 20.0);
    c.hifreq = (float)o.num("hifreq", 8000.0);
    c.use_power = (int)o.num("usePower", 0);
    c.mel_htk_compatible = (int)o.num("htkcompatible", 1);
    if (lower(o.str("specScale", "mel")) != "mel") o.err = "[" + mel->name + ":cMelspec] only specScale = mel is expressible";
    if (lower(o.str("bwMethod", "lr")) != "lr") o.err = "[" + mel->name + ":cMelspec] only bwMethod = lr is expressible";
    o.require("inverse", 0, 0); o.require("showFbank", 0, 0); o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
    level = lvl(mel, "writer.dmLevel");
  }
  std::map<std::string, std::vector<Col>> levels;        // what each level of the rest of the graph holds
  std::string cep_name;
  if (mf) {                                             // src/lldcore/mfcc.cpp:33-44
    OptReader o(*mf);
    if (!wired(mf, level)) return false;
    c.first_mfcc = (int)o.num("firstMfcc", 1);
    c.last_mfcc = o.has("lastMfcc") ? (int)o.num("lastMfcc", 12) : c.first_mfcc + (int)o.num("nMfcc", 12) - 1;
    c.cep_lifter = (float)o.num("cepLifter", 22.0);
    c.mfcc_htk_compatible = (int)o.num("htkcompatible", 1);
    c.melfloor = (float)o.num("melfloor", 0.00000001);
    o.require("doLog", 1, 1); o.require("inverse", 0, 0); o.require("printDctBaseFunctions", 0, 0); o.require("processArrayFields", 1, 1);
    if (o.has("nameAppend") && o.str("nameAppend", "mfcc") != "mfcc") o.err = "[" + mf->name + ":cMfcc] nameAppend must stay 'mfcc'";
    if (!o.finish(kBenign)) { err = o.err; return false; }
    if (c.first_mfcc < 0 || c.last_mfcc < c.first_mfcc) { err = "[" + mf->name + ":cMfcc] bad firstMfcc / lastMfcc"; return false; }
    std::vector<Col> cols;
    for (int i = c.first_mfcc; i <= c.last_mfcc; ++i) cols.push_back(Col{0, i, 0, false});
    levels[lvl(mf, "writer.dmLevel")] = cols;
    cep_name = "pcm_fftMag_mfcc";
  } else {                                              // src/lldcore/plp.cpp:45-67
    OptReader o(*pl);
    if (!wired(pl, level)) return false;
    c.plp_lp_order = (int)o.num("lpOrder", 5);
    const int first_cc = (int)o.num("firstCC", 1);
    int last_cc = (int)o.num("lastCC", -1);
    const int n_ceps = (int)o.num("nCeps", -1);
    // where the component stops (plp.cpp:132-139: doLpToCeps switches doLP on, doLP switches doIDFT on): all three off = the
    // auditory spectrum itself (config/audspec), all three on = PLP-CC (config/plp); the cuts in between exist as operators only
    const int do_idft = (int)o.num("doIDFT", 1), do_lp = (int)o.num("doLP", 1), do_ceps = (int)o.num("doLpToCeps", 1);
    p.audspec = !do_idft && !do_lp && !do_ceps;
    if (p.audspec && !audspec_set) {
      err = "[" + pl->name + ":cPlp] doIDFT = 0, doLP = 0, doLpToCeps = 0 (the auditory spectrum) is not mapped by plain -C -- this file runs as --set audspec -C <file>";
      return false;
    }
    if (!p.audspec) {
      if (last_cc < 0) last_cc = n_ceps < 0 ? c.plp_lp_order : n_ceps;
      if (last_cc != c.plp_lp_order || first_cc < 0 || first_cc > 1) o.err = "[" + pl->name + ":cPlp] only firstCC = 0|1 with lastCC = lpOrder is expressible";
    }
    c.first_mfcc = first_cc;                            // (the auditory-spectrum chain does not read lpOrder, firstCC, lastCC, nCeps, cepLifter:
    c.last_mfcc = c.plp_lp_order;                       //  they have no effect on that output, measured on the binary)
    c.cep_lifter = (float)o.num("cepLifter", 0.0);
    c.plp_compression = (float)o.num("compression", 0.33);
    if ((int)o.num("htkcompatible", 1) != 1)
      o.err = "[" + pl->name + ":cPlp] htkcompatible = 0 is not expressible on the fused path (melfloor 1.0 and the HTK equal-loudness curve are built)";
    // the branch the fused kernels implement is the one of config/plp and config/audspec: power mel spectrum in, no log / inverse log
    o.require("doLog", 0, 1); o.require("doAud", 1, 1); o.require("RASTA", 0, 0); o.require("newRASTA", 0, 0);
    o.require("doInvLog", 0, 1);
    if (o.err.empty() && !p.audspec) {
      if (do_lp && !do_ceps)
        o.err = "[" + pl->name + ":cPlp] doLP = 1 with doLpToCeps = 0 (the LP coefficients) is not expressible on the fused path (the per-component operators have it)";
      else if (do_idft && !do_lp && !do_ceps)
        o.err = "[" + pl->name + ":cPlp] doIDFT = 1 with doLP = 0 (the autocorrelation) is not expressible on the fused path (the per-component operators have it)";
      else { o.require("doIDFT", 1, 1); o.require("doLP", 1, 1); o.require("doLpToCeps", 1, 1); }
    }
    o.require("processArrayFields", 1, 1);
    if (!o.finish(kBenign)) { err = o.err; return false; }
    std::vector<Col> cols;
    if (p.audspec) {                                    // one column per band: the static block of SMILEHIP_CHAIN_AUDSPEC
      if (!c.use_power) { err = "[" + mel->name + ":cMelspec] usePower = 0 is not expressible in front of a cPlp (it reads a power mel spectrum)"; return false; }
      if (en) { err = "[" + en->name + ":cEnergy] is not built for the auditory-spectrum chain"; return false; }
      if (by_type.count("cFullinputMean")) { err = "[" + by_type["cFullinputMean"][0]->name + ":cFullinputMean] is not built for the auditory-spectrum chain"; return false; }
      c.chain_kind = SMILEHIP_CHAIN_AUDSPEC;
      p.plp = false;
      for (int i = 0; i < c.n_bands; ++i) cols.push_back(Col{0, i, 0, false});
      cep_name = "audSpec";
    } else {
      for (int i = first_cc; i <= c.plp_lp_order; ++i) cols.push_back(Col{0, i, 0, false});
      cep_name = "PlpCC";
    }
    levels[lvl(pl, "writer.dmLevel")] = cols;
  }
  c.append_log_energy = 0;
  if (en) {                                             // src/lldcore/energy.cpp:33-44: HTK log energy of the raw frame
    OptReader o(*en);
    if (!wired(en, frames_level)) return false;
    o.require("htkcompatible", 1, 0); o.require("log", 1, 1); o.require("rms", 0, 1); o.require("energy2", 0, 0);
    o.require("escaleLog", 1, 1); o.require("ebiasLog", 0, 0); o.require("processArrayFields", 0, 0);
    if (o.str("nameAppend", "energy") != "energy") o.err = "[" + en->name + ":cEnergy] nameAppend must stay 'energy'";
    if (!o.finish(kBenign)) { err = o.err; return false; }
    levels[lvl(en, "writer.dmLevel")] = {Col{1, 0, 0, false}};
    c.append_log_energy = 1;
  }
  // the rest, as soon as the levels a component reads are known: cFullinputMean, cDeltaRegression, cVectorConcat
  int delta_win = -1;
  std::string delta_suffix = "de";
  std::vector<const ConfInstance *> pending;
  for (const ConfInstance &i : f.inst)
    if (i.type == "cFullinputMean" || i.type == "cDeltaRegression" || i.type == "cVectorConcat") pending.push_back(&i);
  while (!pending.empty()) {
    bool progress = false;
    for (size_t pi = 0; pi < pending.size(); ++pi) {
      const ConfInstance &i = *pending[pi];
      std::vector<Col> in;
      bool ready = true;
      for (const std::string &l : split_levels(lvl(&i, "reader.dmLevel"))) {
        auto it = levels.find(l);
        if (it == levels.end()) { ready = false; break; }
        in.insert(in.end(), it->second.begin(), it->second.end());
      }
      if (!ready) continue;
      OptReader o(i);
      if (i.type == "cFullinputMean") {                   // src/dspcore/fullinputMean.cpp:35-45
        if (lower(o.str("meanNorm", "amean")) != "amean") o.err = "[" + i.name + ":cFullinputMean] only meanNorm = amean is expressible";
        o.require("mvn", 0, 0); o.require("symmSubtract", 0, 0); o.require("subtractClipToZero", 0, 0); o.require("specEnorm", 0, 0);
        o.require("htkLogEnorm", 0, 0); o.require("multiLoopMode", 0, 0); o.require("excludeZeros", 0, 0);
        for (Col &cc : in) {
          if (cc.delta != 0 || cc.kind != 0) o.err = "[" + i.name + ":cFullinputMean] mean normalisation is expressible on the static cepstra only";
          cc.cms = true;
        }
      } else if (i.type == "cDeltaRegression") {          // src/dspcore/deltaRegression.cpp:34-41
        const int w = (int)o.num("deltawin", 2);
        if (delta_win >= 0 && w != delta_win) o.err = "[" + i.name + ":cDeltaRegression] all delta stages must share one deltawin";
        delta_win = w;
        o.require("absOutput", 0, 0); o.require("halfWaveRect", 0, 0); o.require("onlyInSegments", 0, 0); o.require("relativeDelta", 0, 0);
        o.require("noPostEOIprocessing", 0, 0);
        delta_suffix = o.str("nameAppend", "de");
        o.str("zeroSegBound", "1");
        for (Col &cc : in) {
          if (cc.cms) o.err = "[" + i.name + ":cDeltaRegression] deltas of the mean-normalised level are not expressible (take them from the un-normalised level)";
          ++cc.delta;
        }
      } else {
        o.str("includeSingleElementFields", "0"); o.str("processArrayFields", "1");
      }
      if (!o.finish(kBenign)) { err = o.err; return false; }
      levels[lvl(&i, "writer.dmLevel")] = in;
      pending.erase(pending.begin() + (long)pi);
      progress = true;
      break;
    }
    if (!progress) {
      err = "[" + pending[0]->name + ":" + pending[0]->type + "] reads level '" + lvl(pending[0], "reader.dmLevel") + "', which the cepstral chain does not produce";
      return false;
    }
  }
  {
    const int n_cep_ = p.audspec ? c.n_bands : (p.plp ? c.plp_lp_order - c.first_mfcc + 1 : c.last_mfcc - c.first_mfcc + 1);
    for (const auto &kv : levels) {
      std::vector<int> cols;
      bool plain = true;
      for (const Col &cc : kv.second) {
        if (cc.delta != 0 || cc.cms) { plain = false; break; }
        cols.push_back(cc.kind == 1 ? n_cep_ : cc.index - (p.audspec ? 0 : c.first_mfcc));
      }
      if (plain && !cols.empty()) p.static_levels[kv.first] = cols;
    }
  }
  // what the sink reads
  if (!any_sink) { err = "the graph has no sink"; return false; }
  std::vector<Col> outc;
  for (const std::string &l : split_levels(lvl(any_sink, "reader.dmLevel"))) {
    auto it = levels.find(l);
    if (it == levels.end()) { err = "[" + any_sink->name + ":" + any_sink->type + "] reads level '" + l + "', which the cepstral chain does not produce"; return false; }
    outc.insert(outc.end(), it->second.begin(), it->second.end());
  }
  // every other active sink must read the same levels (the fused path writes one output matrix; a sink on a stage level or on
  // another combination would silently get nothing), and the source / sink options must be the ones the writers implement
  {
    const std::string want = lvl(any_sink, "reader.dmLevel");
    for (const ConfInstance &i : f.inst) {
      const bool is_sink = i.type.size() > 4 && i.type.compare(i.type.size() - 4, 4, "Sink") == 0;
      const std::string *fn = i.find("filename");
      if (!is_sink || &i == any_sink || !fn || *fn == "?") continue;
      if (lvl(&i, "reader.dmLevel") != want) {
        err = "[" + i.name + ":" + i.type + "] reads '" + lvl(&i, "reader.dmLevel") + "' while [" + any_sink->name + "] reads '" + want +
              "': the fused path writes one output matrix (a sink on a stage level: per-component operators through the plugin)";
        return false;
      }
    }
    std::set<std::string> produced;
    for (const std::string &l : split_levels(want)) produced.insert(l);
    if (!conf_check_io(f, produced, err)) return false;
    p.out_levels = want;
    if (produced.size() == 1)
      for (const ConfInstance &i : f.inst) {
        const std::string *w = i.find("writer.dmLevel");
        if (w && *w == want) { p.out_writer_name = i.name; p.out_writer_type = i.type; }
      }
  }
  // must be [cepstra (, energy)] x (1 + n_delta) blocks, the cepstra of block 0 either all normalised or none
  const int n_cep = p.audspec ? c.n_bands : (p.plp ? c.plp_lp_order - c.first_mfcc + 1 : c.last_mfcc - c.first_mfcc + 1);
  const int block = n_cep + (c.append_log_energy ? 1 : 0);
  if (block == 0 || outc.size() % (size_t)block != 0 || outc.size() / (size_t)block > 3) {
    err = "the sink's columns are not [static | delta | acceleration] blocks of the cepstral chain";
    return false;
  }
  c.n_delta = (int)(outc.size() / (size_t)block) - 1;
  c.delta_win = delta_win < 0 ? 2 : delta_win;
  c.cms = outc[0].cms ? 1 : 0;
  for (size_t k = 0; k < outc.size(); ++k) {
    const int b = (int)(k / (size_t)block), j = (int)(k % (size_t)block);
    const Col &cc = outc[k];
    const bool want_energy = c.append_log_energy && j == n_cep;
    const int first = p.audspec ? 0 : c.first_mfcc;
    const bool ok = cc.delta == b && (want_energy ? cc.kind == 1 : (cc.kind == 0 && cc.index == first + j)) &&
                    cc.cms == (b == 0 && !want_energy && c.cms);
    if (!ok) { err = "the sink's column order is not [cepstra, energy | their deltas | their accelerations]"; return false; }
  }
  if (!c.append_log_energy && en) { err = "cEnergy is computed but not written"; return false; }
  // names as the reference's data memory builds them (field name + [index]); parmKind of the file's own HTK sink
  const char *sfx[3] = {"", "_", "_"};
  for (int b = 0; b <= c.n_delta; ++b) {
    std::string suffix;
    for (int q = 0; q < b; ++q) suffix += std::string(sfx[1]) + delta_suffix;
    for (int j = 0; j < n_cep; ++j) {
      char idx[32];
      snprintf(idx, sizeof(idx), "[%d]", (p.plp || p.audspec) ? j : c.first_mfcc + j);
      p.lld_names.push_back(cep_name + suffix + idx);
    }
    if (c.append_log_energy) p.lld_names.push_back("pcm_LOGenergy" + suffix);
  }
  p.parm_kind = 9;
  if (htk_sink) {
    const std::string *pk = htk_sink->find("parmKind");
    if (pk) p.parm_kind = atoi(pk->c_str());
  }
  std::ostringstream d;
  if (p.audspec) {
    d << "auditory-spectrum chain: " << c.frame_size_sec * 1e3 << " ms / " << c.frame_step_sec * 1e3 << " ms frames, " << c.n_bands << " bands "
      << c.lofreq << "-" << c.hifreq << " Hz, compression " << c.plp_compression << ", " << c.n_delta << " delta stage(s) of deltawin " << c.delta_win
      << "; lpOrder, firstCC, lastCC, nCeps and cepLifter of [" << pl->name << ":cPlp] are accepted and ignored (no effect on the auditory spectrum)";
    p.describe = d.str();
    return true;
  }
  d << (p.plp ? "PLP" : "MFCC") << " chain: " << c.frame_size_sec * 1e3 << " ms / " << c.frame_step_sec * 1e3 << " ms frames, " << c.n_bands
    << " bands " << c.lofreq << "-" << c.hifreq << " Hz, " << n_cep << " cepstra" << (c.append_log_energy ? " + log energy" : "")
    << (c.cms ? ", mean-normalised" : "") << ", " << c.n_delta << " delta stage(s)";
  p.describe = d.str();
  return true;
}

}  // namespace smilehip_host
