"""The scratch block of a set call (boringssl_amd/csrc/set_scratch.h): the
carver and the two layouts built on it, DtlsSetLayout and QuicSetLayout,
compiled for the host into a stand-alone program under AddressSanitizer and
UBSan, with malloc as the allocator.  For every shape -- n on both sides of the
256-record workgroup, one and several runs, both DTLS AD strides, seal and open
-- every array is aligned to its element type (the QUIC tags to 16 bytes), the
arrays lie inside the block and do not overlap, the flag word and the runs'
maxima are contiguous, and the block is exactly as large as the expression the
hand-carved layouts used.  Every byte of every array is written, so a layout
that reaches past its block is the sanitizer's to report.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "set_scratch.h"
using namespace bssl_amd;

struct Array {
  const char *name;
  const void *p;
  size_t bytes, align;
};
#define ARRAY(l, field, count, align) \
  Array { #field, (l).field, (size_t)(count) * sizeof(*(l).field), align }

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      failures++;                   \
      printf("FAIL %s: ", #cond);   \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
    }                               \
  } while (0)

static void check_block(const char *what, void *block, size_t bytes, size_t expected,
                        std::vector<Array> arrays) {
  CHECK(block != nullptr, "%s", what);
  if (!block) return;
  CHECK(bytes == expected, "%s: %zu bytes, expected %zu", what, bytes, expected);
  const uintptr_t lo = (uintptr_t)block, hi = lo + bytes;
  size_t sum = 0;
  for (const Array &a : arrays) {
    const uintptr_t p = (uintptr_t)a.p;
    CHECK(p % a.align == 0, "%s.%s", what, a.name);
    CHECK(p >= lo && p + a.bytes <= hi, "%s.%s outside the block", what, a.name);
    memset(const_cast<void *>(a.p), 0xa5, a.bytes);
    sum += a.bytes;
  }
  CHECK(sum == bytes, "%s: arrays %zu bytes, block %zu", what, sum, bytes);
  std::sort(arrays.begin(), arrays.end(),
            [](const Array &a, const Array &b) { return (uintptr_t)a.p < (uintptr_t)b.p; });
  for (size_t k = 0; k + 1 < arrays.size(); k++)
    CHECK((uintptr_t)arrays[k].p + arrays[k].bytes <= (uintptr_t)arrays[k + 1].p, "%s.%s overlaps %s",
          what, arrays[k].name, arrays[k + 1].name);
  free(block);
}

int main() {
  const uint64_t ns[] = {1, 255, 256, 257}, all_runs[] = {1, 3};
  const uint32_t strides[] = {5, 13};
  char what[96];
  for (uint64_t n : ns)
    for (uint64_t runs : all_runs) {
      for (uint32_t ad_stride : strides)
        for (int open = 0; open < 2; open++) {
          snprintf(what, sizeof(what), "dtls n=%llu runs=%llu ad=%u open=%d", (unsigned long long)n,
                   (unsigned long long)runs, ad_stride, open);
          DtlsSetLayout l(n, runs, ad_stride, open != 0);
          size_t bytes = 0;
          void *block = carve_block(&l, malloc, &bytes);
          // The hand-carved layout's size, as it was written.
          const uint64_t nb = open ? (n + 255) / 256 : 0, wruns = open ? runs : 0;
          uint64_t table_slots = 0;
          if (open)
            for (table_slots = 512; table_slots < 2 * n;) table_slots *= 2;
          const uint64_t words8 = 3 * n + 1 + 7 * wruns + nb;
          const uint64_t words4 = 2 * n + runs + nb + table_slots;
          const size_t expected = 8 * words8 + 4 * words4 + n * (12 + ad_stride + 3);
          CHECK(l.table_slots == table_slots, "%s", what);
          CHECK((void *)l.flag == (void *)l.zeroed && l.run_max == l.zeroed + 1 &&
                    l.zeroed_bytes == 8 * (1 + wruns),
                "%s: zeroed", what);
          check_block(what, block, bytes, expected,
                      {ARRAY(l, frag_len, n, 8), ARRAY(l, seqs, n, 8), ARRAY(l, ad_len, n, 8),
                       ARRAY(l, zeroed, 1, 8), ARRAY(l, run_max, wruns, 8), ARRAY(l, old, 6 * wruns, 8),
                       ARRAY(l, block_s, nb, 8), ARRAY(l, key_index, n, 4), ARRAY(l, run_of, n, 4),
                       ARRAY(l, run_won, runs, 4), ARRAY(l, block_r, nb, 4),
                       ARRAY(l, table, table_slots, 4), ARRAY(l, nonce, 12 * n, 1),
                       ARRAY(l, ad, ad_stride * n, 1), ARRAY(l, valid, n, 1), ARRAY(l, status, n, 1),
                       ARRAY(l, types, n, 1)});
        }
      snprintf(what, sizeof(what), "quic n=%llu runs=%llu", (unsigned long long)n,
               (unsigned long long)runs);
      QuicSetLayout q(n, runs);
      size_t bytes = 0;
      void *block = carve_block(&q, malloc, &bytes);
      const size_t expected = n * (4 * 8 + 16 + 2 * 4 + 12 + 2) + 8 + 4 * runs;
      CHECK((void *)q.flag == (void *)q.zeroed && q.zeroed_bytes == 8, "%s: zeroed", what);
      check_block(what, block, bytes, expected,
                  {ARRAY(q, body_off, n, 8), ARRAY(q, body_len, n, 8), ARRAY(q, ad_len, n, 8),
                   ARRAY(q, pns, n, 8), ARRAY(q, tags, 16 * n, 16), ARRAY(q, zeroed, 1, 8),
                   ARRAY(q, key_index, n, 4), ARRAY(q, run_of, n, 4), ARRAY(q, run_won, runs, 4),
                   ARRAY(q, nonce, 12 * n, 1), ARRAY(q, valid, n, 1), ARRAY(q, status, n, 1)});
    }
  // A failed allocation: null, nothing carved into.
  DtlsSetLayout l(4, 1, 13, true);
  size_t bytes = 0;
  CHECK(carve_block(&l, [](size_t) -> void * { return nullptr; }, &bytes) == nullptr, "no block");
  printf("%d failures\n", failures);
  return failures != 0;
}
"""


def test_set_scratch_layout(tmp_path):
    src, exe = tmp_path / "layout.cc", tmp_path / "layout"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "boringssl_amd", "csrc"), str(src),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "0 failures", r.stdout
