// Host-only check of the argument refusals of csrc/swiglu.hip (no device is touched: every call below returns before a launch).
// Build with the host sanitizers and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -x hip \
//       tools/dbg/swiglu_args_test.cpp octic_vits_amd/csrc/swiglu.hip -o /tmp/swiglu_args_test && /tmp/swiglu_args_test
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/octic_hip.h"

static int fails = 0;
#define EXPECT(call, want)                                                           \
  do {                                                                               \
    const int got_ = (call);                                                         \
    if (got_ != (want)) {                                                            \
      std::printf("FAIL %s:%d  %s = %d, want %d\n", __FILE__, __LINE__, #call, got_, (want)); \
      ++fails;                                                                       \
    }                                                                                \
  } while (0)

int main() {
  // real host buffers (16-byte aligned), so that a refusal path that did touch its operands would be seen by the sanitizers
  std::vector<uint16_t> bx(4 * 40 + 16), bg(4 * 24 + 16), ba(4 * 24 + 16), bd(4 * 40 + 16);
  auto al = [](std::vector<uint16_t>& v) { return (uint16_t*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); };
  uint16_t *x = al(bx), *g = al(bg), *a = al(ba), *d = al(bd);
  EXPECT(octic_swiglu_blocks() > 0, 1);
  // forward
  EXPECT(octic_swiglu_fwd(x, 24, a, 12, 4, 12, nullptr), OCTIC_ESHAPE);        // H % 8
  EXPECT(octic_swiglu_fwd(x, 32, a, 16, 4, 0, nullptr), OCTIC_ESHAPE);
  EXPECT(octic_swiglu_fwd(x, 32, a, 16, -1, 16, nullptr), OCTIC_ESHAPE);
  EXPECT(octic_swiglu_fwd(x, 24, a, 16, 4, 16, nullptr), OCTIC_ESHAPE);        // ld12 < 2H
  EXPECT(octic_swiglu_fwd(x, 32, a, 8, 4, 16, nullptr), OCTIC_ESHAPE);         // lda < H
  EXPECT(octic_swiglu_fwd(x, 33, a, 16, 4, 16, nullptr), OCTIC_EALIGN);        // odd row stride
  EXPECT(octic_swiglu_fwd(x, 32, a, 20, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_fwd(x + 1, 32, a, 16, 4, 16, nullptr), OCTIC_EALIGN);    // one element off
  EXPECT(octic_swiglu_fwd(x, 32, a + 1, 16, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_fwd(nullptr, 32, a, 16, 4, 16, nullptr), OCTIC_ENULL);
  EXPECT(octic_swiglu_fwd(x, 32, nullptr, 16, 4, 16, nullptr), OCTIC_ENULL);
  EXPECT(octic_swiglu_fwd(nullptr, 33, nullptr, 3, 0, 12, nullptr), OCTIC_OK);  // rows == 0: nothing to do
  // backward
  EXPECT(octic_swiglu_bwd(x, 24, g, 12, d, 24, nullptr, 4, 12, nullptr), OCTIC_ESHAPE);
  EXPECT(octic_swiglu_bwd(x, 32, g, 16, d, 32, nullptr, -1, 16, nullptr), OCTIC_ESHAPE);
  EXPECT(octic_swiglu_bwd(x, 24, g, 16, d, 32, nullptr, 4, 16, nullptr), OCTIC_ESHAPE);
  EXPECT(octic_swiglu_bwd(x, 32, g, 8, d, 32, nullptr, 4, 16, nullptr), OCTIC_ESHAPE);
  EXPECT(octic_swiglu_bwd(x, 32, g, 16, d, 24, nullptr, 4, 16, nullptr), OCTIC_ESHAPE);
  EXPECT(octic_swiglu_bwd(x, 40, g, 17, d, 32, nullptr, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_bwd(x, 36, g, 16, d, 32, nullptr, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_bwd(x, 32, g, 16, d, 35, nullptr, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_bwd(x + 1, 32, g, 16, d, 32, nullptr, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_bwd(x, 32, g + 1, 16, d, 32, nullptr, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_bwd(x, 32, g, 16, d + 1, 32, nullptr, 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_bwd(x, 32, g, 16, d, 32, (float*)((char*)d + 2), 4, 16, nullptr), OCTIC_EALIGN);
  EXPECT(octic_swiglu_bwd(nullptr, 32, g, 16, d, 32, nullptr, 4, 16, nullptr), OCTIC_ENULL);
  EXPECT(octic_swiglu_bwd(x, 32, nullptr, 16, d, 32, nullptr, 4, 16, nullptr), OCTIC_ENULL);
  EXPECT(octic_swiglu_bwd(x, 32, g, 16, nullptr, 32, nullptr, 4, 16, nullptr), OCTIC_ENULL);
  EXPECT(octic_swiglu_bwd(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 16, nullptr), OCTIC_OK);
  std::printf(fails ? "swiglu_args_test: %d FAILED\n" : "swiglu_args_test: all refusals as documented\n", fails);
  return fails != 0;
}
