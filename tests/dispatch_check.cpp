// gcm_pick (csrc/gcm_dispatch.h) as plain host C++: compiled and run by tests/test_dispatch_cpu.py.
// Exit status 0: every check held; otherwise the line of the first one that did not.
#include <cstdio>

#include "gcm_dispatch.h"

static int calls;
static int fail_line;
#define CHECK(cond) \
  if (!(cond) && !fail_line) fail_line = __LINE__

int main() {
  // one dimension: f's own value comes back, a non-zero one included
  calls = 0;
  CHECK(gcm_pick([&](auto a) { ++calls; static_assert(a() == 1 || a() == 2 || a() == 4, ""); return 10 + a(); },
                 OneOf<1, 2, 4>{4}) == 14);
  CHECK(calls == 1);
  calls = 0;
  CHECK(gcm_pick([&](auto a) { ++calls; return a() == 1 ? GCM_OK : 99; }, OneOf<1, 2, 4>{1}) == GCM_OK);
  CHECK(calls == 1);

  // two dimensions, the constants usable as template arguments
  calls = 0;
  CHECK(gcm_pick([&](auto a, auto b) { ++calls; return std::integral_constant<int, 100 * a() + b()>::value; },
                 OneOf<32, 64>{64}, OneOf<1, 2, 3>{2}) == 6402);
  CHECK(calls == 1);

  // four dimensions (the fused step's NT, NCT, NHT, N2T), a flag among them
  for (int nt = 1; nt <= 4; ++nt)
    for (int nct = 1; nct <= 2; ++nct)
      for (int flag = 0; flag <= 1; ++flag)
        for (int n2t = 1; n2t <= 2; ++n2t) {
          calls = 0;
          const int rc = gcm_pick(
              [&](auto a, auto b, auto c, auto d) {
                ++calls;
                return 1000 * a() + 100 * b() + 10 * int(bool(c())) + d();
              },
              OneOf<1, 2, 3, 4>{nt}, OneOf<1, 2>{nct}, Flag{flag}, OneOf<1, 2>{n2t});
          CHECK(rc == 1000 * nt + 100 * nct + 10 * flag + n2t);
          CHECK(calls == 1);
        }

  // a miss in the first, a middle and the last dimension: nothing is called
  calls = 0;
  auto f4 = [&](auto, auto, auto, auto) { ++calls; return GCM_OK; };
  CHECK(gcm_pick(f4, OneOf<1, 2, 3, 4>{5}, OneOf<1, 2>{1}, OneOf<1, 2>{1}, OneOf<1, 2>{1}) == GCM_EUNSUPPORTED);
  CHECK(gcm_pick(f4, OneOf<1, 2, 3, 4>{4}, OneOf<1, 2>{1}, OneOf<1, 2>{0}, OneOf<1, 2>{1}) == GCM_EUNSUPPORTED);
  CHECK(gcm_pick(f4, OneOf<1, 2, 3, 4>{4}, OneOf<1, 2>{2}, OneOf<1, 2>{2}, OneOf<1, 2>{3}) == GCM_EUNSUPPORTED);
  CHECK(gcm_pick([&](auto) { ++calls; return GCM_OK; }, OneOf<16, 32>{-16}) == GCM_EUNSUPPORTED);
  CHECK(calls == 0);

  // a constant by hand
  CHECK(f4(gcm_c<1>, gcm_c<2>, gcm_c<1>, gcm_c<2>) == GCM_OK && calls == 1);

  if (fail_line) std::printf("dispatch_check: line %d\n", fail_line);
  return fail_line ? 1 : 0;
}
