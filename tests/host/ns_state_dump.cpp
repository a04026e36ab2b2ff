// Prints what ns_state.h decides, for tests/test_ns_state_cpu.py.
// stdin, one request per line: a word and its numbers
//   stop logvol logz lmax loglstar dead_prev it ncall dlogz logl_max maxiter maxcall
//        -> {"mask": m, "dz": delta ln Z}
//   size plan_bytes runs fixed_bytes n_dead elem.. rows..          -> {"bytes": image_bytes}
//   image what version sizeof_run plan_bytes ndim max_iter runs cap fixed_bytes rows..
//        an image of `runs` runs (one dead-point array of 8 bytes per row) is built in memory, round-tripped through
//        validate, then damaged as `what` says (ok | magic | version | runsize | short1 | cuthdr | rows | plan) and
//        validated again by a reader with the given version / sizeof_run / plan_bytes / ndim / max_iter
//        -> {"code": c, "text": "...", "cap": capacity or 0, "same": header round trip}
// The writer's version, sizeof_run, plan_bytes and ndim are 100, 176, 64 and 5.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ns_state.h"

using namespace dh_ns_state;

static double num() {
  char w[64];
  if (scanf("%63s", w) != 1) exit(2);
  if (!strcmp(w, "inf")) return INFINITY;
  if (!strcmp(w, "-inf")) return -INFINITY;
  return strtod(w, nullptr);
}
static long long whole() {
  long long v;
  if (scanf("%lld", &v) != 1) exit(2);
  return v;
}

int main() {
  char word[32];
  while (scanf("%31s", word) == 1) {
    if (!strcmp(word, "stop")) {
      StopState s;
      StopRule c;
      s.logvol = num();
      s.logz = num();
      s.lmax = num();
      s.loglstar = num();
      s.dead_prev = num();
      s.it = whole();
      s.ncall = whole();
      c.dlogz = num();
      c.logl_max = num();
      c.maxiter = whole();
      c.maxcall = whole();
      printf("{\"mask\": %d, \"dz\": %.17g}\n", stop_mask(s, c), delta_logz(s));
    } else if (!strcmp(word, "size")) {
      Header h;
      memset(&h, 0, sizeof h);
      h.header_bytes = sizeof(Header);
      h.plan_bytes = (uint32_t)whole();
      h.runs = (int32_t)whole();
      h.fixed_bytes = (uint64_t)whole();
      const int nd = (int)whole();
      std::vector<uint32_t> elems((size_t)nd);
      for (auto& e : elems) e = (uint32_t)whole();
      std::vector<int64_t> rows((size_t)h.runs);
      for (auto& r : rows) r = whole();
      printf("{\"bytes\": %llu, \"header\": %zu}\n", (unsigned long long)image_bytes(h, rows.data(), nd, elems.data()),
             sizeof(Header));
    } else if (!strcmp(word, "image")) {
      char what[32];
      if (scanf("%31s", what) != 1) return 2;
      const uint32_t version = (uint32_t)whole(), sizeof_run = (uint32_t)whole(), plan_bytes = (uint32_t)whole();
      const int ndim = (int)whole();
      const int64_t max_iter = whole();
      Header h;
      memset(&h, 0, sizeof h);
      h.magic = kMagic;
      h.version = 100;
      h.sizeof_run = 176;
      h.header_bytes = sizeof(Header);
      h.plan_bytes = 64;
      h.runs = (int32_t)whole();
      h.nlive = 50;
      h.ndim = 5;
      h.queue_size = 8;
      h.cap = whole();
      h.fill = 3;
      h.cube_phase = 1;
      h.n_words = 2;
      h.row_bytes = 8;
      h.fixed_bytes = (uint64_t)whole();
      std::vector<int64_t> rows((size_t)h.runs);
      for (auto& r : rows) r = whole();
      const uint32_t elem = 8;
      std::vector<int64_t> honest = rows;
      for (auto& r : honest) r = r < 0 ? 0 : r > h.cap ? h.cap : r;  // (the bytes an honest writer would have laid down)
      h.total_bytes = image_bytes(h, honest.data(), 1, &elem);
      // an exact-size heap buffer: a read past the end is the sanitizer's to find
      std::vector<unsigned char> img((size_t)h.total_bytes, 0x5a);
      memcpy(img.data(), &h, sizeof h);
      memcpy(img.data() + sizeof h + pad8(h.plan_bytes), rows.data(), rows.size() * 8);
      Header back;
      const int64_t* rp = nullptr;
      int64_t cap = 0;
      int same = 0;
      if (validate(img.data(), img.size(), 100, 176, 64, 5, 0, &back, &rp, &cap) == IMG_OK)
        same = !memcmp(&back, &h, sizeof h) && cap == h.cap && (const unsigned char*)rp == img.data() + sizeof h + pad8(h.plan_bytes);
      size_t n = img.size();
      if (!strcmp(what, "magic")) img[0] ^= 0xff;
      if (!strcmp(what, "version")) img[8] += 1;
      if (!strcmp(what, "runsize")) img[12] += 8;
      if (!strcmp(what, "plan")) img[20] += 8;
      if (!strcmp(what, "short1")) n -= 1;
      if (!strcmp(what, "cuthdr")) n = sizeof(Header) - 8;
      std::vector<unsigned char> cut(img.begin(), img.begin() + (long)n);
      cap = 0;
      const int code = validate(cut.data(), cut.size(), version, sizeof_run, plan_bytes, ndim, max_iter, &back, &rp, &cap);
      printf("{\"code\": %d, \"text\": \"%s\", \"cap\": %lld, \"same\": %d, \"total\": %llu}\n", code, reject_text(code),
             (long long)(code == IMG_OK ? cap : 0), same, (unsigned long long)h.total_bytes);
    } else {
      return 2;
    }
  }
  return 0;
}
