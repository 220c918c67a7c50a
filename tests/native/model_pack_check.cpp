// CPU harness for csrc/model_pack.h (the model loader's host half: blob parsing and the packing of every array a kernel reads).
// Built by tests/test_host_logic.py with -fsanitize=address,undefined and run as a child process.
//
//   model_pack_check BLOB            pack the blob as it is; print the geometry, a line per packed array (name, element size, bytes,
//                                    FNV-1a 64 of its bytes) and the float64 tables' values
//   model_pack_check BLOB CASES      one packing per line of CASES, each on a fresh copy of the blob changed as the line says:
//                                    "shift=1" (the copy starts 1 byte past a 16-byte boundary), "len=N" (cut to N bytes),
//                                    "u32@OFF=VALUE" (the 4 bytes at OFF replaced), "ins@OFF" (one byte inserted at OFF, after
//                                    the replacements); an empty line changes nothing
// Every copy is a heap block of exactly the blob's size, so a read past a truncated blob's end is a sanitizer report.
// Exit code 0 = every case ended with a status (printed); what the sanitizers have to say goes to stderr.
#include "model_pack.h"

#include <cinttypes>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

static uint64_t fnv1a64(const uint8_t *p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

static void report(const ww_packed_model &pm, int rc, bool values) {
  printf("status %d %s\n", rc, pm.err);
  if (rc != WW_OK) return;
  const ww_filter_geom &f = pm.filt;
  printf("geom info kind=%d window=%d n_mel=%d n_bins=%d n_out=%d enc_rows=%d enc_width=%d\n", pm.info.kind, pm.info.window, pm.info.n_mel,
         pm.info.n_bins, pm.info.n_out, pm.info.enc_rows, pm.info.enc_width);
  printf("geom filt n_mel=%d n_bins=%d floor=%a log_off=%a scale=%a total_taps=%d max_len=%d melv_aligned=%d\n", f.n_mel, f.n_bins, f.floor_v,
         f.log_off, f.scale, f.total_taps, f.max_len, f.melv_aligned);
  if (pm.kind == WW_KIND_CRNN) {
    const ww_crnn_geom &c = pm.crnn;
    printf("geom crnn n_mel=%d T=%d C=%d KF=%d KT=%d SF=%d ST=%d PF=%d PT=%d OF=%d OT=%d H=%d NOUT=%d HEAD=%d generic=%d FEATP=%d\n", c.n_mel, c.T,
           c.C, c.KF, c.KT, c.SF, c.ST, c.PF, c.PT, c.OF, c.OT, c.H, c.NOUT, c.HEAD, (int)c.generic, c.FEATP);
  } else {
    const ww_wave_geom &v = pm.wave;
    printf("geom wave T=%d n_mel=%d C=%d S=%d NB=%d NOUT=%d dil=", v.T, v.n_mel, v.C, v.S, v.NB, v.NOUT);
    for (int d : v.dil) printf("%d,", d);
    printf(" order=");
    for (int d : v.order) printf("%d,", d);
    printf(" has_res=");
    for (int d : v.has_res) printf("%d,", d);
    printf("\n");
  }
  size_t end = 0;
  for (const ww_pack_entry &e : pm.table) {
    if (e.off % WW_PACK_ALIGN || e.off < end || e.off + e.bytes > pm.bytes.size()) {
      printf("bad entry %s\n", e.name);
      exit(3);
    }
    end = e.off + e.bytes;
    printf("array %s %u %zu %016" PRIx64 "\n", e.name, e.elt, e.bytes, fnv1a64(pm.bytes.data() + e.off, e.bytes));
    if (values && e.elt == 8) {
      printf("f64 %s", e.name);
      for (size_t i = 0; i < e.bytes / 8; ++i) {
        double d;
        memcpy(&d, pm.bytes.data() + e.off + 8 * i, 8);
        printf(" %.17g", d);
      }
      printf("\n");
    }
  }
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string blob = ss.str();
  if (blob.empty()) return 2;
  std::vector<std::string> cases;
  if (argc > 2) {
    std::ifstream cf(argv[2]);
    for (std::string line; std::getline(cf, line);) cases.push_back(line);
  } else {
    cases.push_back("");
  }
  for (size_t ci = 0; ci < cases.size(); ++ci) {
    std::string work = blob;
    size_t shift = 0, len = blob.size();
    std::istringstream toks(cases[ci]);
    for (std::string t; toks >> t;) {
      unsigned long long a = 0, b = 0;
      if (sscanf(t.c_str(), "shift=%llu", &a) == 1) shift = (size_t)a;
      else if (sscanf(t.c_str(), "len=%llu", &a) == 1 && a <= len) len = (size_t)a;
      else if (sscanf(t.c_str(), "u32@%llu=%llu", &a, &b) == 2 && a + 4 <= work.size()) {
        const uint32_t v = (uint32_t)b;
        memcpy(&work[a], &v, 4);
      } else if (sscanf(t.c_str(), "ins@%llu", &a) == 1 && a <= work.size()) {
        work.insert((size_t)a, 1, (char)0xa5);
        ++len;
      } else return 2;
    }
    void *block = nullptr;
    if (posix_memalign(&block, 16, shift + len + (shift + len == 0))) return 2;
    uint8_t *copy = (uint8_t *)block + shift;
    memcpy(copy, work.data(), len);
    ww_packed_model pm;
    const int rc = ww_pack_model(pm, copy, len);
    printf("case %zu\n", ci);
    report(pm, rc, argc == 2);
    free(block);
  }
  fflush(stdout);
  return 0;
}
