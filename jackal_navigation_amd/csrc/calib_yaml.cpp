// calib_yaml.cpp — the calibration file (include/jn_calib.h): the OpenCV FileStorage YAML subset the reference's main() reads
// (point_cloud.cpp:530-540), without OpenCV.  Host only; status codes, never exit.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/jn_calib.h"

namespace {

struct Entry { const char* name; int bit, count, rows, cols; bool either; };   // either: rows x cols or cols x rows
const Entry kEntries[8] = {{"K1", JN_CALIB_K1, 9, 3, 3, false}, {"K2", JN_CALIB_K2, 9, 3, 3, false}, {"D1", JN_CALIB_D1, 5, 1, 5, true},
                           {"D2", JN_CALIB_D2, 5, 1, 5, true},  {"R", JN_CALIB_R, 9, 3, 3, false},   {"T", JN_CALIB_T, 3, 3, 1, true},
                           {"XR", JN_CALIB_XR, 9, 3, 3, false}, {"XT", JN_CALIB_XT, 3, 3, 1, true}};

struct Parser {
  std::string s;
  size_t i = 0;
  void skip_space_and_comments(bool newlines) {
    while (i < s.size()) {
      const char c = s[i];
      if (c == ' ' || c == '\t' || c == '\r' || (newlines && c == '\n')) i++;
      else if (c == '#') while (i < s.size() && s[i] != '\n') i++;
      else break;
    }
  }
  void skip_line() { while (i < s.size() && s[i] != '\n') i++; if (i < s.size()) i++; }
  bool word(std::string& w) {                                   // [A-Za-z0-9_]+
    const size_t b = i;
    while (i < s.size() && (isalnum((unsigned char)s[i]) || s[i] == '_')) i++;
    w = s.substr(b, i - b);
    return i > b;
  }
  bool lit(const char* t) {
    const size_t n = strlen(t);
    if (s.compare(i, n, t) != 0) return false;
    i += n;
    return true;
  }
  bool number(double& v) {
    const char* b = s.c_str() + i;
    // strtod would also take hex, inf and nan: the format has none of them
    const char* p = b;
    if (*p == '+' || *p == '-') p++;
    if (!(isdigit((unsigned char)*p) || (*p == '.' && isdigit((unsigned char)p[1])))) return false;
    if (p[0] == '0' && (p[1] == 'x' || p[1] == 'X')) return false;
    char* e = nullptr;
    v = strtod(b, &e);
    if (e == b) return false;
    i += (size_t)(e - b);
    return true;
  }
  bool list(std::vector<double>& out) {                        // [ v, v, ... ] over any number of lines
    out.clear();
    if (!lit("[")) return false;
    for (;;) {
      skip_space_and_comments(true);
      double v;
      if (!number(v)) return false;
      out.push_back(v);
      if (out.size() > 64) return false;
      skip_space_and_comments(true);
      if (lit("]")) return true;
      if (!lit(",")) return false;
    }
  }
  bool integer_field(const char* key, int& v) {
    skip_space_and_comments(true);
    if (!lit(key)) return false;
    skip_space_and_comments(false);
    if (!lit(":")) return false;
    skip_space_and_comments(false);
    double d;
    if (!number(d) || d != std::floor(d) || d < 0 || d > 1e6) return false;
    v = (int)d;
    return true;
  }
};

bool read_file(const char* path, std::string& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) {
    out.append(buf, n);
    if (out.size() > (1u << 20)) { fclose(f); return false; }
  }
  const bool ok = !ferror(f);
  fclose(f);
  return ok;
}

}  // namespace

extern "C" {

jn_status jn_calib_load_yaml(const char* path, jn_stereo_calib* calib, double XR[9], double XT[3], int32_t* present) {
  if (!path || !calib || !XR || !XT) return JN_ERR_INVALID;
  Parser p;
  if (!read_file(path, p.s)) return JN_ERR_INVALID;
  if (!p.lit("%YAML:1.0") && !p.lit("%YAML 1.0")) return JN_ERR_INVALID;
  p.skip_line();
  p.skip_space_and_comments(true);
  if (p.lit("---")) p.skip_line();
  double val[8][9];
  int mask = 0;
  for (;;) {
    p.skip_space_and_comments(true);
    if (p.i >= p.s.size()) break;
    if (p.lit("...")) break;                                    // end-of-document marker
    std::string key;
    if (!p.word(key)) return JN_ERR_INVALID;
    p.skip_space_and_comments(false);
    if (!p.lit(":")) return JN_ERR_INVALID;
    p.skip_space_and_comments(false);
    int e = -1;
    for (int k = 0; k < 8; k++) if (key == kEntries[k].name) e = k;
    std::vector<double> data;
    int rows = -1, cols = -1;
    if (p.lit("!!opencv-matrix")) {
      std::string dt;
      if (!p.integer_field("rows", rows) || !p.integer_field("cols", cols)) return JN_ERR_INVALID;
      p.skip_space_and_comments(true);
      if (!p.lit("dt")) return JN_ERR_INVALID;
      p.skip_space_and_comments(false);
      if (!p.lit(":")) return JN_ERR_INVALID;
      p.skip_space_and_comments(false);
      if (p.lit("\"")) { if (!p.word(dt) || !p.lit("\"")) return JN_ERR_INVALID; }
      else if (!p.word(dt)) return JN_ERR_INVALID;
      if (dt != "d" && dt != "f") return JN_ERR_INVALID;
      p.skip_space_and_comments(true);
      if (!p.lit("data")) return JN_ERR_INVALID;
      p.skip_space_and_comments(false);
      if (!p.lit(":")) return JN_ERR_INVALID;
      p.skip_space_and_comments(true);
      if (!p.list(data) || (long long)rows * cols != (long long)data.size()) return JN_ERR_INVALID;
    } else if (p.i < p.s.size() && p.s[p.i] == '[') {
      if (!p.list(data)) return JN_ERR_INVALID;
    } else if (e < 0) {
      p.skip_line();                                            // an unknown scalar entry
      continue;
    } else {
      return JN_ERR_INVALID;
    }
    if (e < 0) continue;                                        // an unknown matrix or sequence: skipped
    const Entry& en = kEntries[e];
    if ((mask & en.bit) || (int)data.size() != en.count) return JN_ERR_INVALID;
    if (rows >= 0 && !((rows == en.rows && cols == en.cols) || (en.either && rows == en.cols && cols == en.rows))) return JN_ERR_INVALID;
    for (int k = 0; k < en.count; k++) val[e][k] = data[k];
    mask |= en.bit;
  }
  if ((mask & JN_CALIB_STEREO) != JN_CALIB_STEREO) return JN_ERR_INVALID;
  memcpy(calib->K1, val[0], sizeof calib->K1); memcpy(calib->K2, val[1], sizeof calib->K2);
  memcpy(calib->D1, val[2], sizeof calib->D1); memcpy(calib->D2, val[3], sizeof calib->D2);
  memcpy(calib->R, val[4], sizeof calib->R); memcpy(calib->T, val[5], sizeof calib->T);
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Z[3] = {0, 0, 0};
  memcpy(XR, (mask & JN_CALIB_XR) ? val[6] : I, sizeof I);
  memcpy(XT, (mask & JN_CALIB_XT) ? val[7] : Z, sizeof Z);
  if (present) *present = mask;
  return JN_OK;
}

jn_status jn_calib_save_yaml(const char* path, const jn_stereo_calib* c, const double XR[9], const double XT[3]) {
  if (!path || !c || !XR || !XT) return JN_ERR_INVALID;
  const double* src[8] = {c->K1, c->K2, c->D1, c->D2, c->R, c->T, XR, XT};
  for (int e = 0; e < 8; e++)
    for (int k = 0; k < kEntries[e].count; k++) if (!std::isfinite(src[e][k])) return JN_ERR_INVALID;
  FILE* f = fopen(path, "wb");
  if (!f) return JN_ERR_INVALID;
  fprintf(f, "%%YAML:1.0\n");
  for (int e = 0; e < 8; e++) {
    const Entry& en = kEntries[e];
    fprintf(f, "%s: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: d\n   data: [ ", en.name, en.rows, en.cols);
    for (int k = 0; k < en.count; k++) {
      char num[40];
      snprintf(num, sizeof num, "%.17g", src[e][k]);
      // FileStorage wants a number to look like a real: "1" -> "1."
      if (!strpbrk(num, ".eE")) strcat(num, ".");
      fprintf(f, "%s%s", num, k + 1 < en.count ? (k % 3 == 2 ? ",\n       " : ", ") : " ]\n");
    }
  }
  const bool ok = !ferror(f);
  return (fclose(f) == 0 && ok) ? JN_OK : JN_ERR_INVALID;
}

}  // extern "C"
