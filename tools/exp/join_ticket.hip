// Experiment: what the persistent kernels' join (lstm_cluster_dev.h, cluster_join) costs a launch.  256 workgroups of 256 threads,
// one per CU; thread 0 reads its XCD and takes ONE returning agent-scope fetch_add ticket of that XCD's counter, with
// wall_clock64() (100 MHz) before and after.  Layout (a): the eight counters in 32 bytes of one 128-byte line (words 16..23);
// layout (b): the eight counters 128 bytes apart (words 2112 + 32 x).  Per layout, over 20 launches
// (alternating, after 3 warm-up launches each): the spread between the first and the last ticket's completion, the spread of the
// workgroups' starts (what the dispatcher alone contributes) and the longest single ticket.
//   hipcc --offload-arch=gfx950 -O3 -o join_ticket join_ticket.hip && ./join_ticket
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

#define CHECK(x)                                                                      \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      printf("%s: %s\n", #x, hipGetErrorString(e_));                                  \
      return 1;                                                                       \
    }                                                                                 \
  } while (0)

constexpr int kGrid = 256, kWords = 4096, kLaunches = 20, kWarm = 3;

__global__ __launch_bounds__(256) void join_kernel(unsigned* sync, int base, int stride, unsigned long long* out) {
  __shared__ int s_word;
  if (threadIdx.x == 0) {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    x &= 7;  // (the probe only needs a counter index inside the buffer; the library gives up on x >= 8)
    const unsigned long long t0 = wall_clock64();
    const unsigned ticket = __hip_atomic_fetch_add(sync + base + (int)x * stride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(ticket) : "memory");
    const unsigned long long t1 = wall_clock64();
    out[blockIdx.x * 4 + 0] = t0;
    out[blockIdx.x * 4 + 1] = t1;
    out[blockIdx.x * 4 + 2] = ((unsigned long long)x << 32) | ticket;
    s_word = (int)ticket;
  }
  __syncthreads();
  if (s_word < 0) out[blockIdx.x * 4 + 3] = 1;  // (never: keeps every thread behind the join, like the library's kernels)
}

struct Stat {
  std::vector<double> done, start, longest;
};

static double med(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main() {
  unsigned* sync;
  unsigned long long* out;
  CHECK(hipMalloc(&sync, kWords * sizeof(unsigned)));
  CHECK(hipMalloc(&out, kGrid * 4 * sizeof(unsigned long long)));
  CHECK(hipMemset(sync, 0, kWords * sizeof(unsigned)));
  std::vector<unsigned long long> h(kGrid * 4);
  const int base[2] = {16, 2112}, stride[2] = {1, 32};
  const char* name[2] = {"(a) 8 counters in one 128-byte line (words 16..23)", "(b) one 128-byte line per counter (words 2112 + 32 x)"};
  Stat st[2];
  bool tickets_ok = true;
  for (int it = 0; it < kWarm + kLaunches; ++it)
    for (int l = 0; l < 2; ++l) {
      hipLaunchKernelGGL(join_kernel, dim3(kGrid), dim3(256), 0, 0, sync, base[l], stride[l], out);
      CHECK(hipGetLastError());
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(h.data(), out, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
      unsigned long long s0 = ~0ull, s1 = 0, d0 = ~0ull, d1 = 0, lg = 0;
      int per_xcd[8] = {};
      for (int b = 0; b < kGrid; ++b) {
        const unsigned long long t0 = h[b * 4], t1 = h[b * 4 + 1];
        s0 = std::min(s0, t0), s1 = std::max(s1, t0), d0 = std::min(d0, t1), d1 = std::max(d1, t1), lg = std::max(lg, t1 - t0);
        const unsigned x = (unsigned)(h[b * 4 + 2] >> 32), ticket = (unsigned)h[b * 4 + 2];
        per_xcd[x]++;
        if ((int)(ticket >> 5) != it) tickets_ok = false;  // 32 workgroups per XCD and launch: ticket >> 5 is the launch number
      }
      for (int x = 0; x < 8; ++x)
        if (per_xcd[x] != 32) tickets_ok = false;
      if (it >= kWarm) {
        st[l].done.push_back((d1 - d0) * 0.01), st[l].start.push_back((s1 - s0) * 0.01), st[l].longest.push_back(lg * 0.01);
      }
    }
  printf("join ticket probe: %d workgroups x 256 threads, %d launches per layout (us; 100 MHz clock, 0.01 us resolution)\n", kGrid, kLaunches);
  printf("32 workgroups per XCD and ticket >> 5 == launch number in every launch: %s\n", tickets_ok ? "yes" : "NO");
  double m[2];
  for (int l = 0; l < 2; ++l) {
    printf("%s\n", name[l]);
    printf("  first -> last ticket completed : median %.2f  min %.2f  max %.2f\n", m[l] = med(st[l].done),
           *std::min_element(st[l].done.begin(), st[l].done.end()), *std::max_element(st[l].done.begin(), st[l].done.end()));
    printf("  first -> last workgroup started: median %.2f  min %.2f  max %.2f\n", med(st[l].start),
           *std::min_element(st[l].start.begin(), st[l].start.end()), *std::max_element(st[l].start.begin(), st[l].start.end()));
    printf("  longest single ticket          : median %.2f  min %.2f  max %.2f\n", med(st[l].longest),
           *std::min_element(st[l].longest.begin(), st[l].longest.end()), *std::max_element(st[l].longest.begin(), st[l].longest.end()));
    printf("  per launch, first -> last ticket completed:");
    for (double v : st[l].done) printf(" %.2f", v);
    printf("\n");
  }
  printf("(a) - (b), median spread of the ticket completions: %.2f us\n", m[0] - m[1]);
  return 0;
}
