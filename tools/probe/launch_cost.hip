// Host cost of csrc/launch.h per call after the first, against a bare hipGetDevice (DESIGN.md §5 "Launch setup").
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Ispeaker_diarization_amd/csrc tools/probe/launch_cost.hip \
//     -o tools/probe/launch_cost && tools/probe/launch_cost
#include <chrono>
#include <cstdio>

#include "launch.h"

__global__ void k_empty(int*) {}

template <class F>
static double ns_per(F f, int n) {
  auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i) f();
  return std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n;
}

int main() {
  try {
    const int n = 5000000;
    volatile int sink = 0;
    sd::allow_dynamic_lds<&k_empty>(96 * 1024);
    sink = sd::device_cus();
    for (int r = 0; r < 3; ++r) {
      const double a = ns_per([&] { int d; (void)hipGetDevice(&d); sink = d; }, n);
      const double b = ns_per([&] { sink = sd::device_cus(); }, n);
      const double c = ns_per([&] { sd::allow_dynamic_lds<&k_empty>(96 * 1024); }, n);
      printf("round %d: hipGetDevice %.1f ns, device_cus() %.1f ns, allow_dynamic_lds<>() %.1f ns per call (CUs %d)\n", r, a, b,
             c, (int)sink);
    }
  } catch (const sd::Error& e) {
    printf("error: %s\n", e.msg.c_str());
    return 1;
  }
  return 0;
}
