// CPU harness for the recurrent-cell side of csrc/model_pack.h: CRNN blobs of either cell (GRU | LSTM), H in {16, 32, 48, 64} and a
// head of F in 1..64.  Built by tests/test_rnn_cells_host.py with -fsanitize=address,undefined and run as a child process.
//
//   rnn_pack_check BLOB [CASES]     one packing per line of CASES (none: the blob as it is), each on a fresh heap copy of exactly the
//                                   case's size (a read past a truncated blob's end is a sanitizer report), changed as the line says:
//                                   "len=N" (cut to N bytes), "u32@OFF=VALUE" (the 4 bytes at OFF replaced), "swap@I,J" (entries I and
//                                   J of the section table exchanged: each name then points at the other's payload), "name@I=TEXT"
//                                   (entry I renamed); an empty line changes nothing
// Per case: "status RC TEXT", and for an accepted blob one "rnn ..." line: the geometry words, and what this program itself checked
// on the packed arrays against the blob's sections - wx2 as [2 G H][SEQP] with layer 2's rows in its first 2H columns and zeros
// behind them, wx1p likewise on FEATP, bh1 / bh2 all zero for an LSTM and the blob's values for a GRU, w1 as [F][2H].
// Exit code 0 = every case ended with a status; what the sanitizers have to say goes to stderr.
#include "model_pack.h"

#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

static const ww_pack_entry *find(const ww_packed_model &pm, const char *name) {
  for (const ww_pack_entry &e : pm.table)
    if (strcmp(e.name, name) == 0) return &e;
  return nullptr;
}

static std::vector<float> packed(const ww_packed_model &pm, const char *name) {
  std::vector<float> v;
  if (const ww_pack_entry *e = find(pm, name)) {
    v.resize(e->bytes / 4);
    if (e->bytes) memcpy(v.data(), pm.bytes.data() + e->off, e->bytes);
  }
  return v;
}

// [rows][ld] holds a | b (rows / 2 rows of `width` each) in its first `width` columns and zeros behind them
static bool padded_rows(const std::vector<float> &got, const std::vector<float> &a, const std::vector<float> &b, size_t rows, size_t width, size_t ld) {
  if (got.size() != rows * ld || a.size() != rows / 2 * width || b.size() != a.size()) return false;
  for (size_t r = 0; r < rows; ++r)
    for (size_t k = 0; k < ld; ++k) {
      const float want = k < width ? (r < rows / 2 ? a[r * width + k] : b[(r - rows / 2) * width + k]) : 0.f;
      if (memcmp(&got[r * ld + k], &want, 4) != 0) return false;
    }
  return true;
}

static void report(const ww_packed_model &pm, int rc, const blob_view &bv) {
  printf("status %d %s\n", rc, pm.err);
  if (rc != WW_OK || pm.kind != WW_KIND_CRNN) return;
  const ww_crnn_geom &c = pm.crnn;
  const size_t G = (size_t)(c.CELL == WW_CELL_LSTM ? 4 : 3) * c.H, in1 = (size_t)c.OF * c.C, in2 = 2 * (size_t)c.H;
  std::vector<float> a, b;
  bool wx2 = bv.words("crnn.g2f.wx", a) && bv.words("crnn.g2b.wx", b) && padded_rows(packed(pm, "crnn.wx2"), a, b, 2 * G, in2, c.SEQP);
  bool wx1p = !c.generic || (bv.words("crnn.g1f.wx", a) && bv.words("crnn.g1b.wx", b) && padded_rows(packed(pm, "crnn.wx1p"), a, b, 2 * G, in1, c.FEATP));
  bool bh = true;
  for (int layer = 1; layer <= 2; ++layer) {
    const std::vector<float> got = packed(pm, layer == 1 ? "crnn.bh1" : "crnn.bh2");
    if (c.CELL == WW_CELL_LSTM) {
      bh = bh && got.size() == 2 * G;
      for (float v : got) bh = bh && v == 0.f && !std::signbit(v);
    } else {
      bh = bh && bv.words(layer == 1 ? "crnn.g1f.bh" : "crnn.g2f.bh", a) && bv.words(layer == 1 ? "crnn.g1b.bh" : "crnn.g2b.bh", b) &&
           padded_rows(got, a, b, 2, G, G);
    }
  }
  bool w1 = true;
  if (c.HEAD != WW_HEAD_CTC) w1 = bv.words("crnn.head_w1", a) && packed(pm, "crnn.w1") == a && a.size() == (size_t)c.F * in2 &&
                                  packed(pm, "crnn.b1").size() == (size_t)c.F && packed(pm, "crnn.w2").size() == (size_t)c.NOUT * c.F;
  printf("rnn CELL=%d H=%d F=%d SEQP=%d FEATP=%d generic=%d enc_width=%d wx2=%s wx1p=%s bh=%s w1=%s conv=%s\n", c.CELL, c.H, c.F, c.SEQP, c.FEATP,
         (int)c.generic, pm.info.enc_width, wx2 ? "ok" : "BAD", wx1p ? "ok" : "BAD", bh ? "ok" : "BAD", w1 ? "ok" : "BAD",
         find(pm, c.generic ? "crnn.conv_wt" : "crnn.conv_wL") ? "ok" : "BAD");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string blob = ss.str();
  if (blob.size() < 16) return 2;
  std::vector<std::string> cases;
  if (argc > 2) {
    std::ifstream cf(argv[2]);
    for (std::string line; std::getline(cf, line);) cases.push_back(line);
  } else {
    cases.push_back("");
  }
  for (size_t ci = 0; ci < cases.size(); ++ci) {
    std::string work = blob;
    size_t len = blob.size();
    std::istringstream toks(cases[ci]);
    for (std::string t; toks >> t;) {
      unsigned long long a = 0, b = 0;
      char text[32] = {0};
      if (sscanf(t.c_str(), "len=%llu", &a) == 1 && a <= len) len = (size_t)a;
      else if (sscanf(t.c_str(), "u32@%llu=%llu", &a, &b) == 2 && a + 4 <= work.size()) {
        const uint32_t v = (uint32_t)b;
        memcpy(&work[a], &v, 4);
      } else if (sscanf(t.c_str(), "swap@%llu,%llu", &a, &b) == 2 && 16 + 32 * (a + 1) <= work.size() && 16 + 32 * (b + 1) <= work.size()) {
        char ea[8], eb[8];  // (offset, count) of the two entries: the names stay, the payloads change hands
        memcpy(ea, &work[16 + 32 * a + 24], 8);
        memcpy(eb, &work[16 + 32 * b + 24], 8);
        memcpy(&work[16 + 32 * a + 24], eb, 8);
        memcpy(&work[16 + 32 * b + 24], ea, 8);
      } else if (sscanf(t.c_str(), "name@%llu=%23s", &a, text) == 2 && 16 + 32 * (a + 1) <= work.size()) {
        memset(&work[16 + 32 * a], 0, 24);
        memcpy(&work[16 + 32 * a], text, strlen(text));
      } else return 2;
    }
    uint8_t *copy = (uint8_t *)malloc(len + (len == 0));
    if (!copy) return 2;
    memcpy(copy, work.data(), len);
    ww_packed_model pm;
    const int rc = ww_pack_model(pm, copy, len);
    blob_view bv = {copy, len, 0, 0};
    if (rc == WW_OK) {
      ww_packed_model again;
      if (blob_view::open(again, copy, len, &bv) != WW_OK) return 3;
    }
    printf("case %zu\n", ci);
    report(pm, rc, bv);
    free(copy);
  }
  printf("ok %zu\n", cases.size());
  fflush(stdout);
  return 0;
}
