// Stand-alone host check of csrc/rows.h (no GPU, no library): the rows description's refusals and messages, and the
// column packing. tests/test_rows_cpu.py builds it with the host sanitizers and runs it on the CPU.
#include <cassert>
#include <cstdio>
#include <cstring>

#include "rows.h"

using namespace rvcx;

template <class Fn>
static int refused(const char* want, int code, Fn make) {
  try {
    make();
  } catch (const Error& e) {
    if (e.code == code && std::strstr(e.what(), want)) return 0;
    std::printf("wrong refusal: %d %s (want %d %s)\n", e.code, e.what(), code, want);
    return 1;
  }
  std::printf("not refused: %s\n", want);
  return 1;
}

int main() {
  int bad = 0;
  const int64_t nv[5] = {2720, 4960, 5280, 10080, 16000};
  const Rows r("rmvpe", nv, 5, 16000);
  assert(r.B == 5 && r.n_max == 16000 && r.n_min == 2720 && !r.equal);
  const Rows one("rmvpe", nv, 1, 10);  // one row: the stride is not looked at
  assert(one.equal && one.n_max == 2720 && one.n_min == 2720);
  const int64_t same[3] = {700, 700, 700};
  assert(Rows("hubert", same, 3, 700).equal);
  const Rows eq("fcpe", 13920, 3, 13920);
  assert(eq.equal && eq.n_min == 13920 && eq.n_max == 13920 && eq.B == 3);
  bad += refused("rmvpe: batch < 1", RVCX_E_INVALID, [&] { Rows("rmvpe", nv, 0, 16000); });
  bad += refused("rmvpe: batch < 1", RVCX_E_INVALID, [&] { Rows("rmvpe", nv, -3, 16000); });
  bad += refused("fcpe: batch < 1", RVCX_E_INVALID, [&] { Rows("fcpe", 100, 0, 100); });
  bad += refused("rmvpe: row stride shorter than the longest row", RVCX_E_INVALID, [&] { Rows("rmvpe", nv, 5, 15999); });
  bad += refused("fcpe: row stride shorter than the longest row", RVCX_E_INVALID, [&] { Rows("fcpe", 100, 2, 99); });
  const int64_t zero[2] = {100, 0};
  bad += refused("rvcx_x: bad row length", RVCX_E_INVALID, [&] { Rows("rvcx_x", zero, 2, 100, 1); });
  assert(Rows("rvcx_x", nv, 5, 16000, 1).n_min == 2720);
  LenCols len(3, 4);
  for (int k = 0; k < 3; ++k)
    for (int b = 0; b < 4; ++b) len.at(k, b) = 100 * k + b;
  assert(len.h.size() == 12);
  for (int i = 0; i < 12; ++i) assert(len.h[i] == 100 * (i / 4) + i % 4);
  int32_t dev[12];  // stands in for the device copy: col() is plain pointer arithmetic on it
  std::memcpy(dev, len.h.data(), sizeof(dev));
  len.d = dev;
  assert(len.col(2)[3] == 203 && len.col(0) == dev && len.col(1) == dev + 4);
  assert(LenCols(8, 0).h.empty());
  std::printf(bad ? "FAILED %d\n" : "rows.h host checks passed\n", bad);
  return bad;
}
