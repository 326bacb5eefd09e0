// mpcx_api.cpp -- C-ABI host side of libmpcx.so (see include/mpcx.h).
//
// Owns the bound GPUs (one process drives every GPU of the node, as one mpcium
// node process reuses its preparams for every wallet:
// /root/reference/pkg/mpc/node.go:69,109,170), the per-modulus Montgomery
// constants (what Go's nat.expNNMontgomery recomputes on every call: k0 and
// RR, go:src/math/big/nat.go), the kernel workspaces and staging buffers, and
// launches the gfx950 kernels of mpcx_geom.hip / mpcx_prime.hip. No CPU
// compute fallback: every modexp runs on a GPU or the call fails with an
// error code.
//
// Multi-GPU: a host-buffer batch large enough to fill more than one GPU is cut
// into contiguous operand ranges, one per bound device, run concurrently (one
// host thread per device, each on one of that device's lanes) and gathered
// into the caller's output buffer. Independent operands: no collective, no
// peer traffic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mpcx.h"
#include "mpcx_internal.h"

// per-geometry kernels (mpcx_geom.hip, one translation unit per geometry id)
#define MPCX_GEOM_DECL(g)                                                                              \
  hipError_t mpcx_launch_modexp_g##g(const mpcx::ModexpArgs* a, uint32_t waves, hipStream_t st);     \
  hipError_t mpcx_launch_modexp_multi_g##g(const mpcx::ModexpArgs* segs, const uint32_t* first,      \
                                           uint32_t nsegs, uint32_t waves, int mx, hipStream_t st);  \
  hipError_t mpcx_modexp_occupancy_g##g(int* blocks_per_cu);
#define MPCX_FOR_EACH_GEOM(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)
static_assert(MPCX_NUM_GEOMS == 7, "update MPCX_FOR_EACH_GEOM and build.py GEOMS");
extern "C" {
MPCX_FOR_EACH_GEOM(MPCX_GEOM_DECL)
hipError_t mpcx_launch_drbg(const mpcx::DrbgArgs* a, hipStream_t st);
hipError_t mpcx_launch_prime2c(mpcx::Prime2Args a, hipStream_t st);
hipError_t mpcx_launch_mrc(const mpcx::MrArgs* a, hipStream_t st);
hipError_t mpcx_launch_lucasc(const mpcx::LucasArgs* a, hipStream_t st);
hipError_t mpcx_launch_lucasc_wide(const mpcx::LucasArgs* a, hipStream_t st);
hipError_t mpcx_launch_expsched(const mpcx::ExpSchedArgs* a, hipStream_t st);
hipError_t mpcx_launch_fixedbase_g0(const mpcx::FixedBaseArgs* a, uint32_t blocks, uint32_t split, hipStream_t st);
hipError_t mpcx_launch_fixedbase_g1(const mpcx::FixedBaseArgs* a, uint32_t blocks, uint32_t split, hipStream_t st);
hipError_t mpcx_launch_fixedbase_multi_g0(const mpcx::FixedBaseArgs* segs, const uint32_t* first, uint32_t nsegs,
                                          uint32_t blocks, uint32_t split, hipStream_t st);
hipError_t mpcx_launch_fixedbase_multi_g1(const mpcx::FixedBaseArgs* segs, const uint32_t* first, uint32_t nsegs,
                                          uint32_t blocks, uint32_t split, hipStream_t st);
hipError_t mpcx_launch_sieve(const mpcx::SieveArgs* a, hipStream_t st);
hipError_t mpcx_launch_selftest(uint32_t* d_out, hipStream_t st);
hipError_t mpcx_launch_ec_combine(const uint32_t* sc, const uint32_t* pts, uint32_t* out, const uint32_t* gtab,
                                  uint32_t* ws, uint32_t count, hipStream_t st);
hipError_t mpcx_launch_ec_msm(const uint32_t* a, const uint32_t* sc, const uint32_t* pts, uint32_t* out,
                              const uint32_t* gtab, uint32_t* ws, uint32_t count, uint32_t n_points, hipStream_t st);
hipError_t mpcx_launch_ec_probe(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t count,
                                hipStream_t st);
hipError_t mpcx_launch_ed_msm(const uint32_t* a, const uint32_t* sc, const uint32_t* pts, uint32_t* out,
                              const uint32_t* btab, uint32_t* ws, uint32_t count, uint32_t n_points, hipStream_t st);
hipError_t mpcx_launch_ed_comb_entries(const uint32_t* in, uint32_t* out, uint32_t count, hipStream_t st);
hipError_t mpcx_launch_ed_probe(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t count,
                                hipStream_t st);
hipError_t mpcx_launch_ed_admit(const uint32_t* pts, uint32_t* out, uint8_t* status, uint32_t count, uint32_t clear,
                                hipStream_t st);
}

namespace {
constexpr int kMaxDevices = MPCX_MAX_DEVICES;
}

struct mpcx_modulus_s {
  int cls;
  uint32_t bits;
  uint32_t words;  // normalized length of m in 32-bit words
  uint32_t n0inv;
  uint32_t const_off[MPCX_NUM_GEOMS];  // digit offset of geometry g's block (class members only)
  std::vector<uint32_t> m;
  std::vector<uint32_t> host_const;  // per geometry of the class: 3*L_g digits N, R mod N, R^2 mod N
  std::mutex mu;                     // guards the lazy per-device uploads
  uint32_t* d_const[kMaxDevices] = {};
  // k_modexp_mx (4096-bit class): Toeplitz fragments of m'' and m, built on first use
  std::vector<uint8_t> mx_host;
  uint8_t* d_mx[kMaxDevices] = {};
  // k_modexp_nsq (m = N^2): found out and built at the first launch that could take
  // it (nsq_state 0: not yet looked; 1: m is a perfect square; -1: it is not).
  // nsq_host: N's digits and the entry constants (MPCX_NSQ_CONST_DIGITS), then N's
  // Toeplitz tables in MxN2's shape, as words
  int nsq_state = 0;
  std::vector<uint32_t> nsq_host;
  uint32_t* d_nsq[kMaxDevices] = {};
};

struct mpcx_fixedbase_s {
  mpcx_mod_t mod;
  int geom;                          // main geometry of the modulus class (table layout)
  uint32_t nwin;                     // windows: exponents of up to wbits*nwin bits
  uint32_t wbits;                    // window width (entries per window: 2^wbits)
  // nwin x 2^wbits entries x L digits ([k][p] interleaved); held only until the
  // first device has its copy (a 12-bit table is ~320 MB): further devices copy
  // it device to device
  std::vector<uint32_t> host_table;
  size_t table_words = 0;
  std::mutex mu;
  uint32_t* d_table[kMaxDevices] = {};
};

namespace {

constexpr int kDigitBits = 28;
constexpr uint32_t kM28 = (1u << kDigitBits) - 1u;

thread_local std::string g_err;
std::mutex g_mu;  // options, device binding, shutdown
int g_force_geom = -1;                   // mpcx_set_option("force_geom", g): one geometry for everything
double g_narrow_rounds = 0.15;           // mpcx_set_option("narrow_rounds", 100x): narrow-geometry threshold
int g_geom_policy = 1;                   // 1: 4096-bit class by the launch-time model; 0: thresholds only
int g_fixed_win = 5;                     // widest fixed window for per-operand exponents (4 or 5)
int g_sched_width = MPCX_SCHED_MAX_WIDTH;  // mpcx_set_option("sched_width", w): 0 = Go's fixed window
int g_main_geom[MPCX_NUM_CLASSES] = {MPCX_MAIN_GEOM(0), MPCX_MAIN_GEOM(1), MPCX_MAIN_GEOM(2)};
int g_fb_window = MPCX_FB_WINDOW_BITS;  // mpcx_set_option("fb_window", w): fixed-base comb width of new tables
#ifndef MPCX_FB_SPLIT_DEFAULT
#define MPCX_FB_SPLIT_DEFAULT 0  // A/B builds: -DMPCX_FB_SPLIT_DEFAULT=1 (no window split)
#endif
int g_fb_split = MPCX_FB_SPLIT_DEFAULT;  // mpcx_set_option("fb_split", s): comb waves per workgroup (0: by size)
uint32_t g_split_min = 4096;             // mpcx_set_option("device_split_min", n): operands per device slice
int g_ec_msm_ws_mb = 512;                // mpcx_set_option("ec_msm_ws_mb", mb): k_ec_msm table workspace per launch
bool g_dup_device = false;               // mpcx_set_option("duplicate_device", 1): test hook, see below
#ifndef MPCX_MX_DEFAULT
#define MPCX_MX_DEFAULT 1
#endif
int g_mx = MPCX_MX_DEFAULT;              // mpcx_set_option("mx", 1): geometry-2 batches reduce on the matrix cores
#ifndef MPCX_NSQ_DEFAULT
#define MPCX_NSQ_DEFAULT 1
#endif
int g_nsq = MPCX_NSQ_DEFAULT;            // mpcx_set_option("nsq", 1): a k_modexp_mx batch with m = N^2 and a shared exponent runs k_modexp_nsq
uint32_t g_mx_min = 2048;                // mpcx_set_option("mx_min", n): smallest batch for k_modexp_mx
uint32_t g_mx_seg_min = 64;              // mpcx_set_option("mx_seg_min", n): smallest segment of a k_modexp_multi_mx launch (round 6: 64 vs 256, profiles/r06/segmin*)
double g_mx_step = 0.81;                 // mpcx_set_option("mx_step", 100x): k_modexp_mx's wave-round time / k_modexp's (100: model ignores mx)
double g_geom_tput = 0.0;                // mpcx_set_option("geom_tput", 100x): GPU-share weight of the launch-time model
struct Staging {
  void* ptr = nullptr;
  size_t bytes = 0;
};
// An execution lane: one HIP stream with its own exponentiation-table
// workspace and staging buffers. Host-buffer calls from different threads run
// on different lanes concurrently, so small or partial-round batches (a
// latency-bound Fac-proof group, a 10k-wallet MtA step that fills 40% of the
// wavefront slots) overlap on the GPU instead of queueing behind one lock.
// g_lanes: default 6 (measured; HIP gives a process 4 HW queues by default).
struct Lane {
  std::mutex mu;
  hipStream_t st = nullptr;  // created on first use (non-blocking); or a caller's stream (own_stream false)
  bool own_stream = true;
  // completion event for host waits, created with hipEventBlockingSync: a
  // waiting host thread sleeps instead of spinning a core (a signing run has
  // 4-12 tasks waiting on their launches while others need the CPU)
  hipEvent_t ev = nullptr;
  uint32_t* ws = nullptr;    // exponentiation table workspace
  size_t ws_bytes = 0;
  Staging stage[4];  // bases, exps, out, misc
  // safe-prime step: survivors' p words, survivors' indices, trial-division
  // tables + counters, Fermat passes' p words, their indices, ride-along q +
  // verdicts, k_prime2c's per-item constants (R mod n, meta)
  Staging sieve[8];
  // kernel timing (mpcx_kernel_stats): event pairs around this lane's
  // launches, resolved at the lane's next host wait; guarded by mu like the rest
  struct KEv {
    hipEvent_t a = nullptr, b = nullptr;
  };
  struct KPend {
    KEv ev;
    hipEvent_t ref;
    int dev;
    const char* kind;
    int geom;
    uint32_t ops;
    double alg;
    bool nsq = false;  // a modexp_mx launch that ran k_modexp_nsq
  };
  std::vector<KEv> kev_free;
  std::vector<KPend> kpend;
  // Page-locked bounce buffers for host memory that is not a registered
  // pinned allocation (mpcx_host_alloc): the call copies it here itself and
  // DMAs from here, and D2H results land here and are copied out after the
  // lane's host wait (`post`). No pageable pointer ever reaches
  // hipMemcpyAsync, whose pageable path made a CPU read in the runtime that
  // faulted once (profiles/r04/final3/segv/). Cursors reset at
  // every completed wait; guarded by mu.
  struct Bounce {
    char* p = nullptr;
    size_t cap = 0, used = 0;
    size_t peak = 0;     // largest use since the last lane_wait
    uint32_t quiet = 0;  // lane_waits in a row whose peak stayed under kBounceKeep
  };
  Bounce hin, hout;
  struct Post {
    void* dst;
    const void* src;
    size_t bytes;
  };
  std::vector<Post> post;
  bool pending = false;  // copies queued since the last completed wait
};
constexpr int kMaxLanes = 8;
// lanes in use per device: MPCX_LANES (1..8, read at init) or the "lanes" option;
// default 6 (signing lines +3.5% over 4 on HIP's default 4 HW queues,
// profiles/r02/lanes_ab3/)
std::atomic<int> g_lanes{6};

// One bound GPU.
struct Device {
  int ordinal = -1;
  hipEvent_t kref = nullptr;  // kernel-stats time origin (recorded at each stats reset)
  int num_cus = 0;
  int geom_slots[MPCX_NUM_GEOMS] = {0};  // resident wavefronts per geometry
  Lane lanes[kMaxLanes];
  std::atomic<unsigned> lane_rr{0};
  // Workspaces of the device-buffer entry points, one per caller stream: two
  // asynchronous calls on different streams never share a window table or a
  // shared-exponent schedule.
  std::mutex dev_mu;
  std::map<hipStream_t, std::unique_ptr<Lane>> dev_lanes;
  Lane build_lane;  // fixed-base table builds
  std::atomic<uint64_t> launches{0};  // kernel launches of the batch entry points on this device
  std::mutex ec_mu;            // guards the lazy secp256k1 base-point comb build
  uint32_t* ec_gtab = nullptr;  // d 256^w G, w < 32, 1 <= d <= 255 (affine x, y)
  uint32_t* ed_btab = nullptr;  // Ed25519: d 256^w B, same order (y + x, y - x, 2 d x y)
};
Device g_devs[kMaxDevices];
std::atomic<int> g_ndev{0};
std::atomic<unsigned> g_dev_rr{0};
thread_local int t_sel = 0;    // bound-device index of this thread's device-buffer calls
thread_local int t_hip = -1;   // HIP device this thread is bound to

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(MPCX_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// Registry of this library's page-locked allocations (mpcx_host_alloc):
// [start, start + bytes). A host range entirely inside one is DMA'd
// directly; a range that starts inside one and runs past its end is a caller
// bug and fails loudly (the bounds check of VERDICT r4 item 1); anything
// else is bounced through the lane's own pinned buffer.
struct PinRegistry {
  std::shared_mutex mu;
  std::map<uintptr_t, size_t> ranges;
  void add(const void* p, size_t bytes) {
    std::unique_lock<std::shared_mutex> lk(mu);
    ranges[(uintptr_t)p] = bytes;
  }
  void remove(const void* p) {
    std::unique_lock<std::shared_mutex> lk(mu);
    ranges.erase((uintptr_t)p);
  }
  // 1: inside one pinned allocation; 0: not pinned; -1: overruns one
  int lookup(const void* p, size_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    std::shared_lock<std::shared_mutex> lk(mu);
    auto it = ranges.upper_bound(a);
    if (it == ranges.begin()) return 0;
    --it;
    if (a >= it->first + it->second) return 0;
    return a + bytes <= it->first + it->second ? 1 : -1;
  }
};
PinRegistry g_pins;
// copy statistics (mpcx_copy_stats): bytes DMA'd from/to registered pinned
// memory, bytes bounced through the lanes' buffers, bounce-buffer growth
std::atomic<uint64_t> g_cp_direct{0}, g_cp_bounced{0}, g_cp_bounce_grow{0};

// Launch log (environment MPCX_LAUNCH_LOG=<path>): one CSV line per kernel
// launch of the batch entry points -- kind, geometry, operands, modulus bits,
// longest exponent bits, Go-equivalent algorithmic MACs (SURVEY.md 8(d):
// (E + ceil(E/4)) 2 L^2 per exponentiation, summed over the operands' own
// exponent lengths where the host has them) -- so a kernel trace's per-kernel
// time can be set against the work it did (tools/kernel_frac.py).
double go_macs(uint32_t mod_bits, uint32_t e_bits) {
  const double L = (double)((mod_bits + 31) / 32);
  return ((double)e_bits + (double)((e_bits + 3) / 4)) * 2.0 * L * L;
}
void launch_log(const char* kind, int geom, uint32_t count, uint32_t mod_bits, uint32_t exp_bits, double alg) {
  static std::mutex mu;
  static FILE* f = [] {
    const char* p = std::getenv("MPCX_LAUNCH_LOG");
    FILE* h = p && *p ? std::fopen(p, "w") : nullptr;
    if (h) std::fprintf(h, "kind,geom,operands,modulus_bits,exp_bits,alg_macs\n");
    return h;
  }();
  if (!f) return;
  std::lock_guard<std::mutex> lk(mu);
  std::fprintf(f, "%s,%d,%u,%u,%u,%.0f\n", kind, geom, count, mod_bits, exp_bits, alg);
  std::fflush(f);
}

// Kernel statistics (mpcx_kernel_stats; off until the "kernel_stats" option
// is set): per kernel kind and geometry, launches, operands, Go-equivalent
// algorithmic MACs and GPU time from an event pair around each launch, plus
// the union of all kernels' intervals per device (lanes overlap on the GPU,
// so per-kernel times add up to more than the busy time). A protocol line's
// kernel roofline is alg_macs over that busy time.
std::atomic<bool> g_kstats{false};
struct KAgg {
  uint64_t launches = 0, ops = 0;
  uint64_t nsq = 0;  // of the launches: k_modexp_nsq's (kind modexp_mx only)
  double alg = 0.0, ms = 0.0;
};
std::mutex g_kmu;
std::map<std::pair<std::string, int>, KAgg> g_kagg;
std::vector<std::pair<double, double>> g_kiv[8];  // per device: [start, end) ms from its kref
// MPCX_KTRACE=<file>: one CSV line per timed launch, "dev,kind,geom,ops,t0_ns,t1_ns"
// on the host's CLOCK_MONOTONIC (the kref event's completion time is taken as
// its host time), for tools/timeline.py against libmpcx_host's MPCX_HOST_TRACE
uint64_t g_kref_host_ns[8] = {};
uint64_t mono_ns() {
  timespec ts{};
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}
FILE* ktrace_file() {
  static FILE* f = [] {
    const char* p = std::getenv("MPCX_KTRACE");
    FILE* h = p && *p ? std::fopen(p, "w") : nullptr;
    if (h) std::fprintf(h, "dev,kind,geom,ops,t0_ns,t1_ns\n");
    return h;
  }();
  return f;
}

int kstat_begin(Lane& l) {
  if (!g_kstats.load(std::memory_order_relaxed) || l.kpend.size() >= 512) return -1;
  Lane::KEv ev;
  if (!l.kev_free.empty()) {
    ev = l.kev_free.back();
    l.kev_free.pop_back();
  } else if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) {
    return -1;
  }
  if (hipEventRecord(ev.a, l.st) != hipSuccess) {
    l.kev_free.push_back(ev);
    return -1;
  }
  l.kpend.push_back({ev, nullptr, -1, nullptr, 0, 0, 0.0});
  return (int)l.kpend.size() - 1;
}

void kstat_end(Lane& l, int slot, const Device& d, int dev, const char* kind, int geom, uint32_t ops, double alg,
               bool nsq = false) {
  if (slot < 0) return;
  Lane::KPend& p = l.kpend[(size_t)slot];
  if (!d.kref || hipEventRecord(p.ev.b, l.st) != hipSuccess) {
    l.kev_free.push_back(p.ev);
    l.kpend.erase(l.kpend.begin() + slot);
    return;
  }
  p.ref = d.kref;
  p.dev = dev;
  p.kind = kind;
  p.geom = geom;
  p.ops = ops;
  p.alg = alg;
  p.nsq = nsq;
}

// work of a launch whose operand count is known only after it ran (the
// safe-prime step's sieve survivors): added to its kind without a launch
void kstat_credit(const char* kind, int geom, uint64_t ops, double alg) {
  if (!g_kstats.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lk(g_kmu);
  KAgg& a = g_kagg[{kind, geom}];
  a.ops += ops;
  a.alg += alg;
}

// after the lane's stream drained: every pending pair has completed
void kstat_resolve(Lane& l) {
  std::lock_guard<std::mutex> lk(g_kmu);
  for (auto& p : l.kpend) {
    float ms = 0.f, t0 = 0.f;
    if (p.kind && hipEventElapsedTime(&ms, p.ev.a, p.ev.b) == hipSuccess &&
        hipEventElapsedTime(&t0, p.ref, p.ev.a) == hipSuccess) {
      KAgg& a = g_kagg[{p.kind, p.geom}];
      a.launches += 1;
      a.nsq += p.nsq ? 1 : 0;
      a.ops += p.ops;
      a.alg += p.alg;
      a.ms += ms;
      if (p.dev >= 0 && p.dev < 8) g_kiv[p.dev].push_back({(double)t0, (double)t0 + ms});
      if (FILE* kf = ktrace_file(); kf && p.dev >= 0 && p.dev < 8) {
        const uint64_t b = g_kref_host_ns[p.dev];
        std::fprintf(kf, "%d,%s,%d,%u,%llu,%llu\n", p.dev, p.kind, p.geom, p.ops,
                     (unsigned long long)(b + (uint64_t)(t0 * 1e6)), (unsigned long long)(b + (uint64_t)((t0 + ms) * 1e6)));
      }
    }
    l.kev_free.push_back(p.ev);
  }
  l.kpend.clear();
}

int class_for_bits(uint32_t bits) {
  for (int c = 0; c < MPCX_NUM_CLASSES; ++c)
    if ((int)bits <= MPCX_CLASS_MAXBITS(c)) return c;
  return -1;
}

uint32_t bit_length(const std::vector<uint32_t>& x) {
  for (int i = (int)x.size() - 1; i >= 0; --i)
    if (x[i]) return (uint32_t)(32 * i + (32 - __builtin_clz(x[i])));
  return 0;
}

uint32_t bit_length_words(const uint32_t* x, uint32_t n) {
  for (int i = (int)n - 1; i >= 0; --i)
    if (x[i]) return (uint32_t)(32 * i + (32 - __builtin_clz(x[i])));
  return 0;
}

// x >= m (same length)
bool geq(const std::vector<uint32_t>& x, const std::vector<uint32_t>& m) {
  for (int i = (int)x.size() - 1; i >= 0; --i)
    if (x[i] != m[i]) return x[i] > m[i];
  return true;
}

// 2^k mod m by doubling with conditional subtraction (once per registration).
std::vector<uint32_t> pow2_mod(uint32_t k, const std::vector<uint32_t>& m) {
  const size_t n = m.size();
  std::vector<uint32_t> x(n + 1, 0), mm(m);
  mm.push_back(0);
  x[0] = 1;
  if (n == 1 && m[0] == 1) return std::vector<uint32_t>(n, 0);
  for (uint32_t i = 0; i < k; ++i) {
    uint32_t c = 0;
    for (size_t j = 0; j <= n; ++j) {
      const uint32_t nc = x[j] >> 31;
      x[j] = (x[j] << 1) | c;
      c = nc;
    }
    if (geq(x, mm)) {
      uint64_t br = 0;
      for (size_t j = 0; j <= n; ++j) {
        const uint64_t d = (uint64_t)x[j] - mm[j] - br;
        x[j] = (uint32_t)d;
        br = (d >> 63) & 1;
      }
    }
  }
  x.resize(n);
  return x;
}

std::vector<uint32_t> to_digits(const std::vector<uint32_t>& w, uint32_t L) {
  std::vector<uint32_t> d(L, 0);
  for (uint32_t i = 0; i < L; ++i) {
    const uint32_t bit = i * kDigitBits, wi = bit >> 5, s = bit & 31;
    uint64_t v = 0;
    if (wi < w.size()) v = w[wi];
    if (wi + 1 < w.size()) v |= (uint64_t)w[wi + 1] << 32;
    d[i] = (uint32_t)(v >> s) & kM28;
  }
  return d;
}

// ---- k_modexp_mx constants (mpcx_mx.hpp): m'' = -m^-1 mod R, R = 2^(28 L), and
// the LDS image of the Toeplitz tables of m'' and m (MxShape: per table 16 row
// copies of the reversed radix-2^7 digit string, copy_i[x] = v7[D - x + i]).
// a * b mod 2^(32 n)
static void mul_lo(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n) {
  std::vector<uint64_t> acc(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t carry = 0;
    for (uint32_t j = 0; i + j < n; ++j) {
      const uint64_t t = (uint64_t)a[i] * b[j] + (acc[i + j] & 0xFFFFFFFFu) + carry;
      acc[i + j] = (acc[i + j] & ~0xFFFFFFFFull) | (t & 0xFFFFFFFFu);
      carry = t >> 32;
    }
  }
  for (uint32_t i = 0; i < n; ++i) out[i] = (uint32_t)acc[i];
}

// shape constants of the MX geometry with L digits (geometry 2: 148, geometry 5: 74)
struct MxDims {
  uint32_t n7, d, stride, img;
};
static bool mx_dims(uint32_t L, MxDims* o) {
  if (L == mpcx::MxG2::L) {
    *o = {mpcx::MxG2::N7, mpcx::MxG2::D, mpcx::MxG2::TAB_STRIDE, mpcx::MxG2::IMG_BYTES};
  } else if (L == mpcx::MxG5::L) {
    *o = {mpcx::MxG5::N7, mpcx::MxG5::D, mpcx::MxG5::TAB_STRIDE, mpcx::MxG5::IMG_BYTES};
  } else if (L == mpcx::MxN2::L) {
    *o = {mpcx::MxN2::N7, mpcx::MxN2::D, mpcx::MxN2::TAB_STRIDE, mpcx::MxN2::IMG_BYTES};
  } else {
    return false;
  }
  return true;
}

static void mx_tables(const std::vector<uint32_t>& m, uint32_t L, std::vector<uint8_t>& out) {
  MxDims dm{};
  (void)mx_dims(L, &dm);
  const uint32_t W = (kDigitBits * L + 31) / 32;  // words of R = 2^(28 L)
  std::vector<uint32_t> mm(W, 0), x(W, 0), t(W, 0), u(W, 0);
  for (size_t i = 0; i < m.size() && i < W; ++i) mm[i] = m[i];
  uint32_t inv = mm[0];
  for (int i = 0; i < 5; ++i) inv *= 2u - mm[0] * inv;  // m^-1 mod 2^32
  x[0] = inv;
  // Newton: x <- x (2 - m x) doubles the correct low words
  for (uint32_t prec = 1; prec < W;) {
    const uint32_t np = std::min(2 * prec, W);
    mul_lo(mm.data(), x.data(), t.data(), np);
    uint64_t c = 3;  // t <- 2 - t mod 2^(32 np) = ~t + 1 + 2
    for (uint32_t i = 0; i < np; ++i) {
      const uint64_t v = (uint64_t)(uint32_t)~t[i] + c;
      t[i] = (uint32_t)v;
      c = v >> 32;
    }
    mul_lo(x.data(), t.data(), u.data(), np);
    for (uint32_t i = 0; i < np; ++i) x[i] = u[i];
    prec = np;
  }
  // m'' = -x mod 2^(32 W); its radix-2^7 digits below R
  uint64_t br = 1;
  for (uint32_t i = 0; i < W; ++i) {
    const uint64_t v = (uint64_t)(uint32_t)~x[i] + br;
    x[i] = (uint32_t)v;
    br = v >> 32;
  }
  auto d7 = [](const std::vector<uint32_t>& w, uint32_t d) -> uint8_t {
    const uint32_t bit = 7 * d, wi = bit >> 5, sh = bit & 31;
    uint64_t v = wi < w.size() ? w[wi] : 0;
    if (wi + 1 < w.size()) v |= (uint64_t)w[wi + 1] << 32;
    return (uint8_t)((v >> sh) & 0x7F);
  };
  std::vector<uint8_t> n2(dm.n7), n1(dm.n7);
  std::vector<uint32_t> mv(m);
  for (uint32_t d = 0; d < dm.n7; ++d) {
    n2[d] = d7(x, d);
    n1[d] = d7(mv, d);
  }
  out.assign(dm.img, 0);
  auto fill = [&](const std::vector<uint8_t>& v7, uint8_t* dst) {
    for (int i = 0; i < 16; ++i)
      for (int xx = 0; xx < (int)dm.stride; ++xx) {
        const int idx = (int)dm.d - xx + i;
        if (idx >= 0 && idx < (int)dm.n7) dst[i * dm.stride + xx] = v7[idx];
      }
  };
  fill(n2, out.data());
  fill(n1, out.data() + dm.img / 2);
}

// ---- k_modexp_nsq constants (mpcx_device.hpp): is m a perfect square N^2, and
// the pairs (a, b), a + b N = c mod m with a, b < N, of the entry constants.
// (The bignum class of libmpcx_host is not linked into this library; these run
// once per modulus on word vectors.)
static void trim(std::vector<uint32_t>& x) {
  while (x.size() > 1 && x.back() == 0) x.pop_back();
}
// floor(sqrt(m)) bit by bit (shift and subtract), *exact: m is its square
static std::vector<uint32_t> isqrt_words(const std::vector<uint32_t>& m, bool* exact) {
  const size_t n = m.size();
  std::vector<uint32_t> rem(m), res(n, 0), t(n);
  auto bit_of = [&](uint32_t b) { return std::pair<size_t, uint32_t>(b >> 5, 1u << (b & 31)); };
  for (int b = (int)((bit_length(m) - 1) & ~1u); b >= 0; b -= 2) {
    // t = res + 2^b (bit b of res is clear: res only has bits above b)
    t = res;
    const auto [wi, msk] = bit_of((uint32_t)b);
    t[wi] |= msk;
    bool ge = true;
    for (int i = (int)n - 1; i >= 0; --i)
      if (rem[i] != t[i]) {
        ge = rem[i] > t[i];
        break;
      }
    uint32_t c = 0;  // res >>= 1
    for (int i = (int)n - 1; i >= 0; --i) {
      const uint32_t nc = res[i] & 1u;
      res[i] = (res[i] >> 1) | (c << 31);
      c = nc;
    }
    if (ge) {
      uint64_t br = 0;
      for (size_t i = 0; i < n; ++i) {
        const uint64_t d = (uint64_t)rem[i] - t[i] - br;
        rem[i] = (uint32_t)d;
        br = (d >> 63) & 1;
      }
      res[wi] |= msk;
    }
  }
  *exact = true;
  for (uint32_t w : rem) *exact = *exact && w == 0;
  trim(res);
  return res;
}
// x = q n + r by shift and subtract (x < n^2: q, r < n)
static void divmod_words(const std::vector<uint32_t>& x, const std::vector<uint32_t>& n, std::vector<uint32_t>* q,
                         std::vector<uint32_t>* r) {
  const size_t k = n.size();
  std::vector<uint32_t> rem(k + 1, 0), nn(n);
  nn.push_back(0);
  q->assign(x.size(), 0);
  for (int b = (int)(32 * x.size()) - 1; b >= 0; --b) {
    uint32_t c = (x[(size_t)b >> 5] >> (b & 31)) & 1u;
    for (size_t i = 0; i <= k; ++i) {
      const uint32_t nc = rem[i] >> 31;
      rem[i] = (rem[i] << 1) | c;
      c = nc;
    }
    if (geq(rem, nn)) {
      uint64_t br = 0;
      for (size_t i = 0; i <= k; ++i) {
        const uint64_t d = (uint64_t)rem[i] - nn[i] - br;
        rem[i] = (uint32_t)d;
        br = (d >> 63) & 1;
      }
      (*q)[(size_t)b >> 5] |= 1u << (b & 31);
    }
  }
  rem.resize(k);
  *r = rem;
}
// m a perfect square N^2 of the 4096-bit class: out <- N's digits, the pairs of R^2
// and 2^MPCX_NSQ_SPLIT_BITS R^2 mod m (R = 2^(28 MxN2::L)), N's Toeplitz tables
static bool nsq_build(const std::vector<uint32_t>& m, std::vector<uint32_t>& out) {
  constexpr uint32_t L = mpcx::MxN2::L;
  if ((m[0] & 7u) != 1u) return false;  // an odd square is 1 mod 8
  bool exact = false;
  const std::vector<uint32_t> n = isqrt_words(m, &exact);
  // R = 2^2128 > 2^80 N keeps every intermediate of the pair product in 76 digits
  if (!exact || bit_length(n) > 2048 || bit_length(n) < 1025) return false;
  out.clear();
  const auto nd = to_digits(n, L);
  out.insert(out.end(), nd.begin(), nd.end());
  for (uint32_t extra : {0u, (uint32_t)MPCX_NSQ_SPLIT_BITS}) {
    std::vector<uint32_t> c = pow2_mod(2 * kDigitBits * L + extra, m), a, b;
    divmod_words(c, n, &b, &a);
    const auto ad = to_digits(a, L), bd = to_digits(b, L);
    out.insert(out.end(), ad.begin(), ad.end());
    out.insert(out.end(), bd.begin(), bd.end());
  }
  std::vector<uint8_t> img;
  mx_tables(n, L, img);
  const size_t at = out.size();
  out.resize(at + img.size() / 4);
  std::memcpy(out.data() + at, img.data(), img.size());
  return true;
}

hipError_t mpcx_launch_modexp(int geom, const mpcx::ModexpArgs* a, uint32_t waves, hipStream_t st) {
  switch (geom) {
#define MPCX_CASE(g) \
  case g:            \
    return mpcx_launch_modexp_g##g(a, waves, st);
    MPCX_FOR_EACH_GEOM(MPCX_CASE)
#undef MPCX_CASE
    default:
      return hipErrorInvalidValue;
  }
}

// mx: segments laid out in MX_WG-wavefront workgroups (first[] counts workgroups), k_modexp_multi_mx
hipError_t mpcx_launch_modexp_multi(int geom, const mpcx::ModexpArgs* segs, const uint32_t* first, uint32_t nsegs,
                                    uint32_t waves, int mx, hipStream_t st) {
  switch (geom) {
#define MPCX_CASE(g) \
  case g:            \
    return mpcx_launch_modexp_multi_g##g(segs, first, nsegs, waves, mx, st);
    MPCX_FOR_EACH_GEOM(MPCX_CASE)
#undef MPCX_CASE
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t mpcx_modexp_occupancy(int geom, int* blocks_per_cu) {
  switch (geom) {
#define MPCX_CASE(g) \
  case g:            \
    return mpcx_modexp_occupancy_g##g(blocks_per_cu);
    MPCX_FOR_EACH_GEOM(MPCX_CASE)
#undef MPCX_CASE
    default:
      return hipErrorInvalidValue;
  }
}

// HIP's current device is per thread: every entry point binds its thread to
// the device it submits to.
int bind(const Device& d) {
  if (t_hip != d.ordinal) {
    hipError_t e = hipSetDevice(d.ordinal);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    t_hip = d.ordinal;
  }
  return MPCX_OK;
}

int ndev_or_fail() {
  const int n = g_ndev.load(std::memory_order_acquire);
  if (n <= 0) return -fail(MPCX_ENODEV, "mpcx_init() has not been called");
  return n;
}

// The device this thread's device-buffer calls use (mpcx_select_device).
int selected(Device** out) {
  const int n = ndev_or_fail();
  if (n < 0) return -n;
  if (t_sel < 0 || t_sel >= n) return fail(MPCX_EINVAL, "selected device %d not bound (%d bound)", t_sel, n);
  *out = &g_devs[t_sel];
  return bind(**out);
}

// A free lane of device d (round-robin start, first one not in use), else wait for one.
Lane& acquire_lane(Device& d, std::unique_lock<std::mutex>& lk) {
  const unsigned start = d.lane_rr.fetch_add(1, std::memory_order_relaxed);
  const int nl = g_lanes.load(std::memory_order_relaxed);
  for (int i = 0; i < nl; ++i) {
    Lane& l = d.lanes[(start + i) % nl];
    std::unique_lock<std::mutex> t(l.mu, std::try_to_lock);
    if (t.owns_lock()) {
      lk = std::move(t);
      return l;
    }
  }
  Lane& l = d.lanes[start % nl];
  lk = std::unique_lock<std::mutex>(l.mu);
  return l;
}

int lane_stream(Lane& l) {
  if (!l.st && l.own_stream) {
    hipError_t e = hipStreamCreateWithFlags(&l.st, hipStreamNonBlocking);
    if (e != hipSuccess) {
      l.st = nullptr;
      return hip_fail(e, "hipStreamCreate(lane)");
    }
  }
  if (!l.ev) {
    hipError_t e = hipEventCreateWithFlags(&l.ev, hipEventBlockingSync | hipEventDisableTiming);
    if (e != hipSuccess) {
      l.ev = nullptr;
      return hip_fail(e, "hipEventCreate(lane)");
    }
  }
  return MPCX_OK;
}

// Wait until the lane's stream has drained. Default: poll the lane's event
// with a sleep that backs off from 20 to 100 us -- hipEventSynchronize, even
// on a hipEventBlockingSync event, spins inside the HSA runtime before it
// sleeps, and a signing run keeps 4-12 host threads waiting on launches of a
// few ms each: those spins were a third of the process's CPU time
// (profiles/r03/sample1). The added latency is <= 100 us per launch.
// MPCX_LANE_WAIT=event: hipEventSynchronize; =stream: hipStreamSynchronize.
// A bounce buffer grown past kBounceKeep by a large request is released (to the
// deferred-free list: hipHostFree synchronises the device) once kBounceQuiet
// lane waits in a row stayed under kBounceKeep, so one large copy does not pin
// its 1.25x for the life of the lane. Lane idle (used == 0).
constexpr size_t kBounceKeep = (size_t)64 << 20;
constexpr uint32_t kBounceQuiet = 256;
void retire_pinned(char* p, size_t bytes);
void bounce_trim(Lane& l) {
  for (Lane::Bounce* b : {&l.hin, &l.hout}) {
    if (b->cap <= kBounceKeep) {
      b->peak = 0;
      continue;
    }
    b->quiet = b->peak <= kBounceKeep ? b->quiet + 1 : 0;
    b->peak = 0;
    if (b->quiet >= kBounceQuiet) {
      retire_pinned(b->p, b->cap);
      *b = Lane::Bounce{};
    }
  }
}

int lane_wait(Lane& l) {
  static const int mode = [] {
    const char* e = std::getenv("MPCX_LANE_WAIT");
    return !e ? 0 : std::strcmp(e, "event") == 0 ? 1 : std::strcmp(e, "stream") == 0 ? 2 : 0;
  }();
  hipError_t e;
  if (mode == 2) {
    e = hipStreamSynchronize(l.st);
  } else {
    e = hipEventRecord(l.ev, l.st);
    if (e == hipSuccess && mode == 1) {
      e = hipEventSynchronize(l.ev);
    } else if (e == hipSuccess) {
      for (int us = 20;; us = std::min(100, us + us / 2)) {
        e = hipEventQuery(l.ev);
        if (e != hipErrorNotReady) break;
        std::this_thread::sleep_for(std::chrono::microseconds(us));
      }
    }
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(l.st);  // nothing of this call may still read or write host memory
    l.post.clear();
    l.hin.used = l.hout.used = 0;
    l.pending = false;
    return hip_fail(e, "lane wait");
  }
  // bounced results to their destinations, then the bounce buffers are free
  for (const auto& p : l.post) std::memcpy(p.dst, p.src, p.bytes);
  l.post.clear();
  l.hin.used = l.hout.used = 0;
  l.pending = false;
  bounce_trim(l);
  if (!l.kpend.empty()) kstat_resolve(l);
  return MPCX_OK;
}

// A call that fails after queueing copies on its lane drains the lane before
// it returns: those copies read or write the caller's buffers, which the
// caller frees or reuses as soon as it sees the error (VERDICT r4 item 1,
// ADVICE r4). Declared after the lane's lock, so it runs before the unlock.
struct LaneDrain {
  Lane& l;
  explicit LaneDrain(Lane& lane) : l(lane) {}
  ~LaneDrain() {
    if (!l.pending) return;
    if (l.st) (void)hipStreamSynchronize(l.st);
    l.post.clear();  // the call failed: its results are not delivered
    l.hin.used = l.hout.used = 0;
    l.pending = false;
  }
  LaneDrain(const LaneDrain&) = delete;
  LaneDrain& operator=(const LaneDrain&) = delete;
};

// `bytes` of lane bounce buffer b. When it is full, the lane's queued work
// is waited for first (copies may still read the in-buffer; bounced results
// are delivered), then the buffer grows if one request needs more.
void retire_pinned(char* p, size_t bytes);
int bounce_reserve(Lane& l, Lane::Bounce& b, size_t bytes, char** out) {
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (b.used + need > b.cap) {
    if (l.hin.used || l.hout.used) {
      hipError_t e = hipStreamSynchronize(l.st);
      if (e != hipSuccess) return hip_fail(e, "bounce-buffer wait");
      for (const auto& p : l.post) std::memcpy(p.dst, p.src, p.bytes);
      l.post.clear();
      l.hin.used = l.hout.used = 0;
    }
    if (need > b.cap) {
      if (b.p) retire_pinned(b.p, b.cap);
      b.p = nullptr;
      b.cap = 0;
      const size_t want = std::max<size_t>({need + need / 4, (size_t)1 << 20});
      hipError_t e = hipHostMalloc((void**)&b.p, want, hipHostMallocPortable);
      if (e != hipSuccess) {
        b.p = nullptr;
        return fail(MPCX_ENOMEM, "hipHostMalloc(bounce %zu): %s", want, hipGetErrorString(e));
      }
      b.cap = want;
      g_cp_bounce_grow.fetch_add(1, std::memory_order_relaxed);
    }
  }
  *out = b.p + b.used;
  b.used += need;
  b.peak = std::max(b.peak, b.used);
  return MPCX_OK;
}

// Host-to-device copy on lane l: straight from a registered pinned range,
// else through the lane's bounce buffer (the copy into it is ours, in this
// thread, within the caller's stated range).
int h2d(Lane& l, void* d, const void* h, size_t bytes) {
  if (!bytes) return MPCX_OK;
  const int pin = g_pins.lookup(h, bytes);
  if (pin < 0) return fail(MPCX_EINVAL, "host source of %zu B at %p overruns its pinned allocation", bytes, h);
  const void* src = h;
  if (pin == 0) {
    char* b = nullptr;
    if (int rc = bounce_reserve(l, l.hin, bytes, &b)) return rc;
    std::memcpy(b, h, bytes);
    src = b;
    g_cp_bounced.fetch_add(bytes, std::memory_order_relaxed);
  } else {
    g_cp_direct.fetch_add(bytes, std::memory_order_relaxed);
  }
  l.pending = true;
  hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, l.st);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "copy inputs");
}

// Device-to-host copy on lane l, complete after the lane's next successful
// lane_wait (a bounced result is copied to h by that wait).
int d2h(Lane& l, void* h, const void* d, size_t bytes) {
  if (!bytes) return MPCX_OK;
  const int pin = g_pins.lookup(h, bytes);
  if (pin < 0) return fail(MPCX_EINVAL, "host destination of %zu B at %p overruns its pinned allocation", bytes, h);
  void* dst = h;
  if (pin == 0) {
    char* b = nullptr;
    if (int rc = bounce_reserve(l, l.hout, bytes, &b)) return rc;
    dst = b;
    l.post.push_back({h, b, bytes});
    g_cp_bounced.fetch_add(bytes, std::memory_order_relaxed);
  } else {
    g_cp_direct.fetch_add(bytes, std::memory_order_relaxed);
  }
  l.pending = true;
  hipError_t e = hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, l.st);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "copy results");
}

int d2h_sync(void* h, const void* d, size_t bytes, Lane& l) {
  if (int rc = d2h(l, h, d, bytes)) return rc;
  return lane_wait(l);
}

// Pinned staging for copy_sync: persistent 16-MB chunks handed out under a
// mutex. hipHostFree synchronises the whole device, so a chunk allocated and
// freed per call stalled every lane's in-flight kernels on each modulus, mx
// table or comb-table upload; chunks are now allocated once (one
// per concurrent copier) and kept until mpcx_shutdown.
constexpr size_t kStageChunk = (size_t)16 << 20;
struct StageChunks {
  std::mutex mu;
  std::vector<char*> free_list;
  size_t allocated = 0;
  char* get() {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!free_list.empty()) {
        char* c = free_list.back();
        free_list.pop_back();
        return c;
      }
    }
    char* c = nullptr;
    if (hipHostMalloc((void**)&c, kStageChunk, hipHostMallocPortable) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    ++allocated;
    return c;
  }
  void put(char* c) {
    std::lock_guard<std::mutex> lk(mu);
    free_list.push_back(c);
  }
  void release_all() {  // mpcx_shutdown: no copy in flight
    std::lock_guard<std::mutex> lk(mu);
    for (char* c : free_list) (void)hipHostFree(c);
    free_list.clear();
    allocated = 0;
  }
};
StageChunks g_stage_chunks;

// Pinned buffers retired by a bounce buffer's growth: freed in one batch (one
// device-wide synchronisation) once they pass kRetireMax, or at shutdown,
// rather than one hipHostFree under the lane lock per growth.
constexpr size_t kRetireMax = (size_t)1 << 30;
std::mutex g_retire_mu;
std::vector<std::pair<char*, size_t>> g_retired;
size_t g_retired_bytes = 0;
void retire_pinned(char* p, size_t bytes) {
  std::vector<std::pair<char*, size_t>> out;
  {
    std::lock_guard<std::mutex> lk(g_retire_mu);
    g_retired.push_back({p, bytes});
    g_retired_bytes += bytes;
    if (g_retired_bytes > kRetireMax) {
      out.swap(g_retired);
      g_retired_bytes = 0;
    }
  }
  for (auto& r : out) (void)hipHostFree(r.first);
}
void free_retired() {
  std::lock_guard<std::mutex> lk(g_retire_mu);
  for (auto& r : g_retired) (void)hipHostFree(r.first);
  g_retired.clear();
  g_retired_bytes = 0;
}

// Synchronous copy of a large or one-off host buffer (modulus constants, comb
// tables and their build inputs, the public mpcx_memcpy_* helpers) on stream
// st, through a persistent pinned staging chunk unless the range is registered pinned.
int copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  if (!bytes) return MPCX_OK;
  const void* hp = kind == hipMemcpyHostToDevice ? src : dst;
  const int pin = g_pins.lookup(hp, bytes);
  if (pin < 0) return fail(MPCX_EINVAL, "host range of %zu B at %p overruns its pinned allocation", bytes, hp);
  hipError_t e;
  if (pin == 1) {
    e = hipMemcpyAsync(dst, src, bytes, kind, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? MPCX_OK : hip_fail(e, "copy");
  }
  char* buf = g_stage_chunks.get();
  if (!buf) return fail(MPCX_ENOMEM, "hipHostMalloc(copy chunk %zu)", kStageChunk);
  const size_t cb = std::min(bytes, kStageChunk);
  e = hipSuccess;
  for (size_t off = 0; off < bytes && e == hipSuccess; off += cb) {
    const size_t n = std::min(cb, bytes - off);
    if (kind == hipMemcpyHostToDevice) {
      std::memcpy(buf, (const char*)src + off, n);
      e = hipMemcpyAsync((char*)dst + off, buf, n, kind, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    } else {
      e = hipMemcpyAsync(buf, (const char*)src + off, n, kind, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e == hipSuccess) std::memcpy((char*)dst + off, buf, n);
    }
  }
  g_stage_chunks.put(buf);
  g_cp_bounced.fetch_add(bytes, std::memory_order_relaxed);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "copy");
}

// Buffers grow with headroom: hipFree waits for the whole device, so a size
// that creeps up call by call (a safe-prime step's candidates plus a varying
// ride-along count, a lane's workspace across batch sizes) must not reallocate
// -- and stall every other lane -- on each new maximum.
size_t grown(size_t old_bytes, size_t bytes) {
  return std::max<size_t>({bytes + bytes / 4, old_bytes + old_bytes / 2, (size_t)1 << 20});
}

int ensure_buffer(Staging& s, size_t bytes) {
  if (s.bytes >= bytes && s.ptr) return MPCX_OK;
  const size_t want = grown(s.bytes, bytes);
  if (s.ptr) (void)hipFree(s.ptr);
  s.ptr = nullptr;
  s.bytes = 0;
  hipError_t e = hipMalloc(&s.ptr, want);
  if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
  s.bytes = want;
  return MPCX_OK;
}

int ensure_workspace(Lane& l, size_t bytes) {
  if (l.ws_bytes >= bytes) return MPCX_OK;
  if (l.ws) {
    // the lane's previous kernels may still read the old workspace
    (void)hipStreamSynchronize(l.st);
    (void)hipFree(l.ws);
  }
  const size_t want = grown(l.ws_bytes, bytes);
  l.ws = nullptr;
  l.ws_bytes = 0;
  hipError_t e = hipMalloc((void**)&l.ws, want);
  if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(workspace %zu): %s", want, hipGetErrorString(e));
  l.ws_bytes = want;
  return MPCX_OK;
}

void drop_lane(Lane& l) {
  std::lock_guard<std::mutex> ll(l.mu);
  if (l.st) {
    (void)hipStreamSynchronize(l.st);
    if (l.own_stream) (void)hipStreamDestroy(l.st);
  }
  l.st = nullptr;
  if (l.ev) (void)hipEventDestroy(l.ev);
  l.ev = nullptr;
  for (auto& p : l.kpend) l.kev_free.push_back(p.ev);
  l.kpend.clear();
  for (auto& ev : l.kev_free) {
    (void)hipEventDestroy(ev.a);
    (void)hipEventDestroy(ev.b);
  }
  l.kev_free.clear();
  if (l.ws) (void)hipFree(l.ws);
  l.ws = nullptr;
  l.ws_bytes = 0;
  for (auto& s : l.stage) {
    if (s.ptr) (void)hipFree(s.ptr);
    s = Staging{};
  }
  for (auto& s : l.sieve) {
    if (s.ptr) (void)hipFree(s.ptr);
    s = Staging{};
  }
  for (Lane::Bounce* b : {&l.hin, &l.hout}) {
    if (b->p) (void)hipHostFree(b->p);
    *b = Lane::Bounce{};
  }
  l.post.clear();
  l.pending = false;
}

// Device-buffer workspace of (device, caller stream).
Lane& stream_lane(Device& d, hipStream_t st) {
  std::lock_guard<std::mutex> lk(d.dev_mu);
  auto& p = d.dev_lanes[st];
  if (!p) {
    p.reset(new Lane());
    p->own_stream = false;
    p->st = st;
  }
  return *p;
}

int run_selftest() {
  uint32_t* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, 256 * sizeof(uint32_t));
  if (e != hipSuccess) return hip_fail(e, "selftest alloc");
  e = mpcx_launch_selftest(d, nullptr);
  std::vector<uint32_t> h(256);
  if (e == hipSuccess && copy_sync(h.data(), d, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr) != MPCX_OK)
    e = hipErrorInvalidValue;
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(e, "selftest");
  for (uint32_t l = 0; l < 64; ++l) {
    const uint32_t nxt = l < 63 ? 1000 + l + 1 : 0;
    const uint32_t prv = l > 0 ? 1000 + l - 1 : 0;
    const uint32_t bp = 2000 + (l / 7) * 7;
    const uint64_t acc = (uint64_t)(0xFFFFFFF0u + l) * (0xFFFFFFF7u - l) + 0xFFFFFFFFFFFFull;
    if (h[l] != nxt || h[64 + l] != prv || h[128 + l] != bp || h[192 + l] != (uint32_t)(acc >> 32))
      return fail(MPCX_EHIP,
                  "device self-test failed at lane %u (dpp next %u/%u prev %u/%u bpermute %u/%u mad %u/%u)", l,
                  h[l], nxt, h[64 + l], prv, h[128 + l], bp, h[192 + l], (uint32_t)(acc >> 32));
  }
  return MPCX_OK;
}

// Bind HIP ordinal `ordinal` as the next device (g_mu held).
int bind_new_device(int ordinal) {
  const int n = g_ndev.load();
  // duplicate_device (test hook): bind the ordinal again as one more logical
  // device with its own lanes, constants and workspaces, so the multi-device
  // split / gather paths run concurrently on a one-GPU box
  for (int i = 0; i < n && !g_dup_device; ++i)
    if (g_devs[i].ordinal == ordinal) return MPCX_OK;
  if (n >= kMaxDevices) return fail(MPCX_EINVAL, "more than %d devices", kMaxDevices);
  int vis = 0;
  hipError_t e = hipGetDeviceCount(&vis);
  if (e != hipSuccess || vis <= 0) return fail(MPCX_ENODEV, "no HIP device visible");
  if (ordinal < 0 || ordinal >= vis) return fail(MPCX_EINVAL, "device %d out of range [0,%d)", ordinal, vis);
  e = hipSetDevice(ordinal);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  t_hip = ordinal;
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, ordinal);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MPCX_ENODEV, "device %d is %s; libmpcx is built for gfx950 only", ordinal, prop.gcnArchName);
  Device& d = g_devs[n];
  d.ordinal = ordinal;
  d.num_cus = prop.multiProcessorCount;
  for (int g = 0; g < MPCX_NUM_GEOMS; ++g) {
    int b = 0;
    if (mpcx_modexp_occupancy(g, &b) != hipSuccess || b <= 0) b = 1;
    d.geom_slots[g] = b * d.num_cus;
  }
  int rc = run_selftest();
  if (rc != MPCX_OK) {
    d.ordinal = -1;
    return rc;
  }
  g_ndev.store(n + 1, std::memory_order_release);
  return MPCX_OK;
}

// The modulus constants on bound device di (uploaded on first use there).
int mod_const(mpcx_mod_t mod, int di, const uint32_t** out) {
  std::lock_guard<std::mutex> lk(mod->mu);
  if (!mod->d_const[di]) {
    uint32_t* p = nullptr;
    hipError_t e = hipMalloc((void**)&p, mod->host_const.size() * sizeof(uint32_t));
    if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(modulus): %s", hipGetErrorString(e));
    if (int rc = copy_sync(p, mod->host_const.data(), mod->host_const.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, nullptr)) {
      (void)hipFree(p);
      return rc;
    }
    mod->d_const[di] = p;
  }
  *out = mod->d_const[di];
  return MPCX_OK;
}

int mx_const(mpcx_mod_t mod, int di, const uint8_t** out) {
  std::lock_guard<std::mutex> lk(mod->mu);
  if (!mod->d_mx[di]) {
    if (mod->mx_host.empty()) mx_tables(mod->m, (uint32_t)MPCX_GEOM_L(MPCX_MAIN_GEOM(mod->cls)), mod->mx_host);
    uint8_t* p = nullptr;
    hipError_t e = hipMalloc((void**)&p, mod->mx_host.size());
    if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(mx tables): %s", hipGetErrorString(e));
    if (int rc = copy_sync(p, mod->mx_host.data(), mod->mx_host.size(), hipMemcpyHostToDevice, nullptr)) {
      (void)hipFree(p);
      return rc;
    }
    mod->d_mx[di] = p;
  }
  *out = mod->d_mx[di];
  return MPCX_OK;
}

// k_modexp_nsq's constants of mod on bound device di, *out = nullptr when mod is no
// perfect square (looked at once, at the first launch that asks)
int nsq_const(mpcx_mod_t mod, int di, const uint32_t** out) {
  std::lock_guard<std::mutex> lk(mod->mu);
  *out = nullptr;
  if (mod->nsq_state == 0) mod->nsq_state = nsq_build(mod->m, mod->nsq_host) ? 1 : -1;
  if (mod->nsq_state < 0) return MPCX_OK;
  if (!mod->d_nsq[di]) {
    uint32_t* p = nullptr;
    const size_t bytes = mod->nsq_host.size() * sizeof(uint32_t);
    hipError_t e = hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(nsq constants): %s", hipGetErrorString(e));
    if (int rc = copy_sync(p, mod->nsq_host.data(), bytes, hipMemcpyHostToDevice, nullptr)) {
      (void)hipFree(p);
      return rc;
    }
    mod->d_nsq[di] = p;
  }
  *out = mod->d_nsq[di];
  return MPCX_OK;
}

int fb_table(mpcx_fb_t fb, int di, const uint32_t** out) {
  std::lock_guard<std::mutex> lk(fb->mu);
  if (!fb->d_table[di]) {
    uint32_t* p = nullptr;
    const size_t bytes = fb->table_words * sizeof(uint32_t);
    hipError_t e = hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(fixed-base table %zu B)", bytes);
    if (!fb->host_table.empty()) {
      const int rc = copy_sync(p, fb->host_table.data(), bytes, hipMemcpyHostToDevice, nullptr);
      e = rc ? hipErrorInvalidValue : hipSuccess;
      if (rc == MPCX_OK) std::vector<uint32_t>().swap(fb->host_table);  // the device copy is the master now
    } else {
      int src = -1;
      for (int j = 0; j < kMaxDevices && src < 0; ++j)
        if (fb->d_table[j]) src = j;
      // device-to-device copies return before they complete, and the lanes'
      // non-blocking streams are not ordered after the null stream: wait for
      // the copy before any launch may read the table
      e = src < 0 ? hipErrorInvalidValue
                  : hipMemcpyPeerAsync(p, g_devs[di].ordinal, fb->d_table[src], g_devs[src].ordinal, bytes, nullptr);
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
      (void)hipFree(p);
      return hip_fail(e, "upload fixed-base table");
    }
    fb->d_table[di] = p;
  }
  *out = fb->d_table[di];
  return MPCX_OK;
}

// Slice plan of a batch over n_dev devices (mpcx_partition): one contiguous
// operand range per device when every range gets at least min_slice
// operands, else one range.
uint32_t partition(uint32_t count, int n_dev, uint32_t min_slice, uint32_t* first, uint32_t* cnt) {
  uint32_t slices = n_dev > 0 ? (uint32_t)n_dev : 1u;
  if (min_slice == 0) slices = 1;
  else slices = std::min<uint32_t>(slices, std::max<uint32_t>(1, count / min_slice));
  const uint32_t per = (count + slices - 1) / std::max<uint32_t>(slices, 1);
  uint32_t used = 0;
  for (uint32_t s = 0; s < slices; ++s) {
    const uint32_t f = std::min(count, s * per), c = std::min(count, f + per) - f;
    if (first) first[s] = f;
    if (cnt) cnt[s] = c;
    used = s + 1;
  }
  return used;
}

// Runs fn(device index, first, n) over [0, count) by the partition plan:
// several slices run concurrently, one host thread per device, and gather by
// writing disjoint output ranges; a single range runs on one device chosen
// round-robin, so concurrent callers spread over the node's GPUs. The first
// failing slice's status and message are returned on the calling thread.
int run_sliced(uint32_t count, uint32_t min_slice, const std::function<int(int, uint32_t, uint32_t)>& fn) {
  const int n = ndev_or_fail();
  if (n < 0) return -n;
  uint32_t first[kMaxDevices], cnt[kMaxDevices];
  const uint32_t slices = partition(count, n, min_slice, first, cnt);
  if (slices <= 1) {
    const int di = (int)(g_dev_rr.fetch_add(1, std::memory_order_relaxed) % (unsigned)n);
    int rc = bind(g_devs[di]);
    return rc ? rc : fn(di, 0, count);
  }
  std::vector<int> rcs(slices, MPCX_OK);
  std::vector<std::string> msgs(slices);
  std::vector<std::thread> th;
  for (uint32_t s = 0; s < slices; ++s) {
    th.emplace_back([&, s] {
      int rc = bind(g_devs[s]);
      if (!rc) rc = fn((int)s, first[s], cnt[s]);
      rcs[s] = rc;
      if (rc) msgs[s] = g_err;
    });
  }
  for (auto& t : th) t.join();
  for (uint32_t s = 0; s < slices; ++s)
    if (rcs[s]) {
      g_err = msgs[s];
      return rcs[s];
    }
  return MPCX_OK;
}

// Can geometry g serve modulus mod? R = 2^(28 L) > 4m, and every base and
// multiplier below R (almost-Montgomery entry mont(x, R^2) < 2m needs x < R).
// The class width is 2^(32 class words); a geometry whose R is below it (the
// lane-pair geometry 5: 2^2072 in a 2080-bit class) needs the caller's check of
// the operands (ops_fit).
bool geom_serves(int g, const mpcx_modulus_s* mod, bool ops_fit) {
  const uint32_t rb = (uint32_t)MPCX_GEOM_RBITS(g);
  if (mod->bits + 2u > rb) return false;
  return ops_fit || rb >= 32u * (uint32_t)MPCX_CLASS_WORDS(mod->cls);
}

// every one of count operands of `words` words below 2^rbits (null: none)
bool host_ops_below(const uint32_t* x, uint32_t count, uint32_t words, uint32_t rbits) {
  if (!x || 32u * words <= rbits) return true;
  const uint32_t w0 = rbits / 32u, sh = rbits % 32u;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t* v = x + (size_t)i * words;
    if (sh && (v[w0] >> sh)) return false;
    for (uint32_t w = w0 + (sh ? 1u : 0u); w < words; ++w)
      if (v[w]) return false;
  }
  return true;
}

// the main geometry of mod's class, or the class's full-width geometry when
// the main one cannot serve this modulus / these operands
int main_geom_for(const mpcx_modulus_s* mod, bool ops_fit) {
  const int g = g_main_geom[mod->cls];
  return geom_serves(g, mod, ops_fit) ? g : MPCX_FULL_GEOM(mod->cls);
}

// ---- launch plan of the modexp batch entry points (single and multi batch)

// Does a launch in geometry g of `total` operands run on the matrix cores?
// A single batch runs k_modexp_mx: the 4096-bit main geometry (mx >= 1), the
// 2048-bit lane pair only on request (mx = 2: it measured slower,
// profiles/r05/mx/g5/). A multi-batch launch runs k_modexp_multi_mx: geometry 2
// only, when the launch is large and its smallest non-empty segment min_seg
// fills at least one workgroup's worth of its tables (the single batch has no
// segment rule).
bool runs_on_mx(int g, uint32_t total, uint32_t min_seg, bool multi) {
  const bool has_kernel = g == 2 || (g == 5 && !multi && g_mx >= 2);
  return g_mx && has_kernel && total >= g_mx_min && (!multi || min_seg >= g_mx_seg_min);
}

// Can montmul_mx in geometry g serve modulus mod? Its result is (T + q m) / R + m with
// |q| <= R/2 (1 + 2^-10): at most A B / R + (3/2 + 2^-11) m, so operands below 2.01 m
// give a result below 2.01 m only if R >= 8m. R > 4m, which the CIOS product needs
// (geom_serves), is not enough: with R = 4m + 4 the values of a squaring chain grow
// past R within a few products (tests/test_mx_model_cpu.py). Geometry 2 always has
// R = 2^4144 >= 2^48 m; geometry 5 (R = 2^2072) leaves its 2070-bit moduli to k_modexp.
bool mx_serves(int g, const mpcx_modulus_s* mod) { return mod->bits + 3u <= (uint32_t)MPCX_GEOM_RBITS(g); }

// Launch-time model of the 4096-bit class's geometries, measured on MI355X
// (tools/geom_sweep.py, profiles/r02/geom_sweep/): a launch of W wavefronts
// takes about c0 + s * k with k = ceil(W / SIMDs) wavefronts per SIMD, in units
// of the main geometry's time per wavefront-per-SIMD step. Per operand the main
// geometry does the least work, but its 16 operands per wavefront leave most
// SIMDs idle or one wave short on batches of a fraction of a round; the mid
// geometry (8 operands per wavefront, 3 resident per SIMD) and the narrow one (2
// per wavefront) trade per-operand work for a finer split. x^N mod N^2 for
// 1.25K / 5K / 10K / 20K / 30K / 40K operands: main 49 / 49 / 50 / 91 / 93 / 135 ms,
// mid 32 / 32 / 55 / 83 / 107 / 134 ms, narrow 20 / 41 / 65 / 119 / 175 / 230 ms.
//
// The 2048-bit class keeps the narrow_rounds threshold: the same kind of model
// fitted to its geometries (tools/geom_sweep.py --class 1,
// profiles/r04/geom_sweep_c1/: lane pair 25.4 ms per wavefront-per-SIMD step,
// 4 x 19 at 0.556 and 16 x 5 at 0.226 of it) sent mid-size batches to 4 x 19 and
// measured 7% slower on config 5's concurrent load (profiles/r04/c1model_ab/).
// mx_ok: the main geometry's launch would run on the matrix cores (runs_on_mx),
// whose wave-per-SIMD step is g_mx_step of the CIOS one
// (config 2: 139.5 vs 172.5 ms, profiles/r06/libab1/ vs profiles/r05/s2/).
// g_geom_tput > 0 adds that weight x the launch's share of the GPU's SIMD time
// (s x waves / nsimd) to its latency: under concurrent launches (signing,
// keygen) the SIMDs a geometry occupies are time the other lanes' kernels lose.
int fastest_geom(int cls, uint32_t count, int nsimd, bool mx_ok) {
  struct M {
    int g;
    double c0, s;
  };
  const M ms[3] = {{MPCX_MAIN_GEOM(cls), 0.10, mx_ok ? g_mx_step : 1.0}, {MPCX_MID_GEOM(cls), 0.12, 0.585},
                   {MPCX_NARROW_GEOM(cls), 0.20, 0.245}};
  int best = ms[0].g;
  double tb = 1e300;
  for (const M& m : ms) {
    const uint32_t G = (uint32_t)MPCX_GEOM_G(m.g);
    const double waves = (double)((count + G - 1) / G);
    const double t = m.c0 + m.s * std::ceil(waves / (double)std::max(1, nsimd)) +
                     g_geom_tput * m.s * waves / (double)std::max(1, nsimd);
    if (t < tb) {
      tb = t;
      best = m.g;
    }
  }
  return best;
}

// The one geometry of a launch of `count` operands of class cls (a multi-batch
// launch takes one for all its segments): the forced geometry, or policy 2's
// main, or policy 1's launch-time model, or the thresholds. main_serves /
// forced_serves: the class's main / the forced geometry serves every modulus
// and operand of the launch (geom_serves); otherwise the full-width one runs.
int choose_geom(const Device& dev, int cls, uint32_t count, bool main_serves, bool forced_serves, bool mx_ok) {
  const int gm = main_serves ? g_main_geom[cls] : MPCX_FULL_GEOM(cls);
  const int gn = MPCX_NARROW_GEOM(cls), gmid = MPCX_MID_GEOM(cls);
  if (g_force_geom >= 0 && MPCX_GEOM_CLASS(g_force_geom) == cls)
    return forced_serves ? g_force_geom : MPCX_FULL_GEOM(cls);
  // policy 2, throughput: the main geometry at every size (concurrent launches
  // from other lanes fill the SIMDs a small batch leaves idle)
  if (g_geom_policy == 2) return gm;
  if (g_geom_policy == 1 && gmid >= 0 && gn >= 0) return fastest_geom(cls, count, dev.num_cus * 4, mx_ok && main_serves);
  // Measured on MI355X (profiles/r01): a lone wavefront issues v_mad_u64_u32
  // at ~45% of SIMD peak, so tiny batches (< 0.15 of a round) finish sooner
  // spread over the narrow geometry's 3x more wavefronts; from ~0.3 rounds up
  // the main geometry wins, and a narrow tail launch did not pay (round 1).
  const uint32_t G = (uint32_t)MPCX_GEOM_G(gm);
  const double rounds = (double)((count + G - 1) / G) / (double)std::max(1, dev.geom_slots[gm]);
  if (gn >= 0 && rounds < g_narrow_rounds) return gn;
  return gm;
}

// Width and null checks of one batch's buffers (count > 0: an empty batch's
// may be null). `pre` is "" for the single-batch entry points and "group i: "
// for a multi-batch group; each keeps its own wording (cgo callers log it): the
// single batch's carries the limits, a group's names the field.
int check_batch(const char* pre, const mpcx_modulus_s* mod, uint32_t count, const uint32_t* bases,
                uint32_t base_words, const uint32_t* exps, uint32_t exp_words, const uint32_t* muls,
                uint32_t mul_words, const uint32_t* out, uint32_t out_words) {
  const bool grp = *pre;
  const uint32_t cw = (uint32_t)MPCX_CLASS_WORDS(mod->cls);
  if (base_words == 0 || base_words > cw)
    return grp ? fail(MPCX_EINVAL, "%sbase_words %u", pre, base_words)
               : fail(MPCX_EINVAL, "base_words %u outside [1, %u] (reduce mod m first)", base_words, cw);
  if (muls && (mul_words == 0 || mul_words > cw))
    return grp ? fail(MPCX_EINVAL, "%smul_words", pre)
               : fail(MPCX_EINVAL, "mul_words %u outside [1, %u]", mul_words, cw);
  if (out_words < mod->words)
    return grp ? fail(MPCX_EINVAL, "%sout_words < modulus words", pre)
               : fail(MPCX_EINVAL, "out_words %u < modulus words %u", out_words, mod->words);
  if (count && (!bases || !out || (exp_words && !exps))) return fail(MPCX_EINVAL, "%snull buffer", pre);
  return MPCX_OK;
}

// Go-equivalent MACs of a batch with per-operand exponents: each operand's own
// exponent length (launch log, kernel stats)
double go_macs_sum(uint32_t mod_bits, const uint32_t* exps, uint32_t exp_words, uint32_t count) {
  double alg = 0.0;
  for (uint32_t i = 0; i < count; ++i)
    alg += go_macs(mod_bits, bit_length_words(exps + (size_t)i * exp_words, exp_words));
  return alg;
}

// a shared exponent's sliding-window schedule, built on the launch stream
int launch_expsched(const uint32_t* d_exp, uint32_t exp_words, uint32_t* sched, hipStream_t st) {
  mpcx::ExpSchedArgs sa{};
  sa.exp = d_exp;
  sa.exp_words = exp_words;
  sa.max_width = (uint32_t)g_sched_width;
  sa.sched = sched;
  hipError_t e = mpcx_launch_expsched(&sa, st);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "launch k_expsched");
}

// Kernel arguments of one batch (a k_modexp launch, or one segment of a
// k_modexp_multi launch) in geometry geom. dconst: the modulus's constants on
// the launch's device (mod_const); sched: the shared exponent's schedule or
// nullptr (fixed window); mx_img: the modulus's Toeplitz tables when the launch
// runs on the matrix cores (mx_const), else nullptr; nwaves: the batch's
// wavefronts (read by the mx kernels only).
mpcx::ModexpArgs modexp_args(const mpcx_modulus_s* mod, int geom, const uint32_t* dconst, uint32_t count,
                             const uint32_t* base, uint32_t base_words, const uint32_t* exps, uint32_t exp_words,
                             const uint32_t* mul, uint32_t mul_words, uint32_t* out, uint32_t out_words,
                             uint32_t* table, uint32_t exp_bits, int exp_shared, const uint32_t* sched,
                             const uint8_t* mx_img, uint32_t nwaves) {
  const uint32_t L = (uint32_t)MPCX_GEOM_L(geom);
  mpcx::ModexpArgs a{};
  a.nd = dconst + mod->const_off[geom];
  a.r1d = a.nd + L;
  a.r2d = a.nd + 2 * L;
  a.base = base;
  a.exps = exps;
  a.mul = mul;
  a.out = out;
  a.table = table;
  a.count = count;
  a.base_words = base_words;
  a.exp_words = exp_words;
  a.mul_words = mul ? mul_words : 0;
  a.exp_bits = exp_words ? exp_bits : 0;
  // fixed window: 5 bits for per-operand exponents above 1024 bits (E/5 + 31
  // table products < E/4 + 15 from 320 bits on; measured +2.4-2.6% on 2048- and
  // 4096-bit exponents, profiles/r02/win_ab/), Go's 4 bits otherwise
  a.win_bits = (!exp_shared && a.exp_bits > 1024u && g_fixed_win >= 5) ? 5u : 4u;
  a.out_words = out_words;
  a.n0inv = mod->n0inv;
  a.exp_shared = exp_shared ? 1 : 0;
  a.sched = sched;
  a.mx_img = mx_img;
  a.nwaves = nwaves;
  return a;
}

// ---- the comb pair: mpcx_fixedbase_exp_batch is one group of mpcx_fixedbase_multi_batch's

// One comb group's checks, and the windows its launch processes per base (the
// longest exponent's). `pre` as check_batch's: "" for mpcx_fixedbase_exp_batch,
// "group i: " for a multi-batch group, each with its own wording.
int fb_group_check(const mpcx_fixedbase_group_t& g, const char* pre, uint32_t* nwin) {
  const bool grp = *pre;
  if (g.nbases == 0 || g.nbases > MPCX_FB_MAX_BASES)
    return fail(MPCX_EINVAL, "%snbases %u outside [1, %d]", pre, g.nbases, MPCX_FB_MAX_BASES);
  for (uint32_t t = 0; t < g.nbases; ++t) {
    if (!g.fbs[t]) return fail(MPCX_EINVAL, "%snull fixed base %u", pre, t);
    if (g.fbs[t]->mod != g.fbs[0]->mod) return fail(MPCX_EINVAL, "%sfixed bases of different moduli", pre);
  }
  mpcx_mod_t mod = g.fbs[0]->mod;
  const uint32_t cw = (uint32_t)MPCX_CLASS_WORDS(mod->cls);
  if (g.out_words < mod->words)
    return grp ? fail(MPCX_EINVAL, "%sout_words < modulus words", pre)
               : fail(MPCX_EINVAL, "out_words %u < modulus words %u", g.out_words, mod->words);
  if (g.muls && (g.mul_words == 0 || g.mul_words > cw))
    return grp ? fail(MPCX_EINVAL, "%smul_words", pre)
               : fail(MPCX_EINVAL, "mul_words %u outside [1, %u]", g.mul_words, cw);
  if (g.count == 0) return MPCX_OK;  // an empty group's buffers may be null
  if (!g.out) return fail(MPCX_EINVAL, "%snull output", pre);
  for (uint32_t t = 0; t < g.nbases; ++t) {
    if (g.exp_words[t] && !g.exps[t]) return fail(MPCX_EINVAL, "%snull exponents %u", pre, t);
    uint32_t bits = 0;
    for (uint32_t i = 0; i < g.count && g.exp_words[t]; ++i)
      bits = std::max(bits, bit_length_words(g.exps[t] + (size_t)i * g.exp_words[t], g.exp_words[t]));
    const uint32_t wb = g.fbs[t]->wbits;
    if (bits > g.fbs[t]->nwin * wb)
      return fail(MPCX_EINVAL, "%sexponent of %u bits > fixed-base table's %u", pre, bits, g.fbs[t]->nwin * wb);
    nwin[t] = (bits + wb - 1) / wb;
  }
  return MPCX_OK;
}

// A comb group's work. alg, Go-equivalent (launch log): one Exp per base per
// operand. exec, executed (kernel stats): one product per window of each
// exponent, plus the multiplier's, 2 L^2 MACs each. eb_max: the longest exponent.
struct FbWork {
  double alg = 0.0, exec = 0.0;
  uint32_t eb_max = 0;
};
FbWork fb_group_work(const mpcx_fixedbase_group_t& g) {
  FbWork w;
  const uint32_t bits = g.fbs[0]->mod->bits;
  const double l2 = 2.0 * (double)((bits + 31) / 32) * (double)((bits + 31) / 32);
  for (uint32_t t = 0; t < g.nbases; ++t)
    for (uint32_t i = 0; i < g.count && g.exp_words[t]; ++i) {
      const uint32_t b = bit_length_words(g.exps[t] + (size_t)i * g.exp_words[t], g.exp_words[t]);
      w.alg += go_macs(bits, b);
      w.exec += (double)((b + g.fbs[t]->wbits - 1) / g.fbs[t]->wbits) * l2;
      w.eb_max = std::max(w.eb_max, b);
    }
  if (g.muls) w.exec += (double)g.count * l2;
  return w;
}

// Kernel arguments of one comb group (a k_fixedbase launch, or one segment of a
// k_fixedbase_multi launch) on device di: its exponents, multipliers and
// outputs at d_exps / d_mul / d_out.
int fixedbase_args(const mpcx_fixedbase_group_t& g, int geom, int di, const uint32_t* nwin,
                   const uint32_t* const* d_exps, const uint32_t* d_mul, uint32_t* d_out, mpcx::FixedBaseArgs* out) {
  mpcx_mod_t mod = g.fbs[0]->mod;
  const uint32_t* dconst = nullptr;
  int rc;
  if ((rc = mod_const(mod, di, &dconst))) return rc;
  mpcx::FixedBaseArgs a{};
  a.nd = dconst + mod->const_off[geom];
  a.r1d = a.nd + MPCX_GEOM_L(geom);
  a.r2d = a.nd + 2 * MPCX_GEOM_L(geom);
  for (uint32_t t = 0; t < g.nbases; ++t) {
    if ((rc = fb_table(g.fbs[t], di, &a.tables[t]))) return rc;
    a.exps[t] = d_exps[t];
    a.exp_words[t] = g.exp_words[t];
    a.nwin[t] = nwin[t];
    a.wbits[t] = g.fbs[t]->wbits;
  }
  a.nbases = g.nbases;
  a.mul = g.muls ? d_mul : nullptr;
  a.mul_words = g.muls ? g.mul_words : 0;
  a.out = d_out;
  a.out_words = g.out_words;
  a.count = g.count;
  a.n0inv = mod->n0inv;
  *out = a;
  return MPCX_OK;
}

// The layout (geometry) of a modulus's comb tables: its class's full-width
// geometry. (A lane-pair layout for 2048-bit moduli was 10% faster at 131k
// operands but 24-30% slower at 16k and neutral end to end, where the comb
// batches are small: profiles/r04/fblp/; removed.)
int fb_geom_for(const mpcx_modulus_s* mod) { return MPCX_FULL_GEOM(mod->cls); }
hipError_t launch_fixedbase(int geom, const mpcx::FixedBaseArgs* a, uint32_t blocks, uint32_t split, hipStream_t st) {
  return geom == 0 ? mpcx_launch_fixedbase_g0(a, blocks, split, st) : mpcx_launch_fixedbase_g1(a, blocks, split, st);
}
hipError_t launch_fixedbase_multi(int geom, const mpcx::FixedBaseArgs* segs, const uint32_t* first, uint32_t nsegs,
                                  uint32_t blocks, uint32_t split, hipStream_t st) {
  return geom == 0 ? mpcx_launch_fixedbase_multi_g0(segs, first, nsegs, blocks, split, st)
                   : mpcx_launch_fixedbase_multi_g1(segs, first, nsegs, blocks, split, st);
}

// Wavefronts per comb workgroup (k_fixedbase's window split): the largest of
// 4, 2, 1 that keeps a launch of `blocks` workgroups within kFbSplitWaves
// wavefronts per SIMD, or option "fb_split" when set.
constexpr uint32_t kFbSplitWaves = 4;
uint32_t fb_split_for(const Device& dev, uint32_t blocks) {
  if (g_fb_split) return (uint32_t)g_fb_split;
  const uint64_t cap = (uint64_t)std::max(1, dev.num_cus) * 4u * kFbSplitWaves;
  for (uint32_t s = MPCX_FB_MAX_SPLIT; s > 1; s >>= 1)
    if ((uint64_t)blocks * s <= cap) return s;
  return 1;
}

}  // namespace

extern "C" {

int mpcx_version(void) { return 200; }

int mpcx_get_option(const char* key, int* value) {
  if (!key || !value) return fail(MPCX_EINVAL, "null option or output");
  std::lock_guard<std::mutex> lk(g_mu);
  if (std::strcmp(key, "mx") == 0) {
    *value = g_mx;
  } else if (std::strcmp(key, "nsq") == 0) {
    *value = g_nsq;
  } else if (std::strcmp(key, "mx_min") == 0) {
    *value = (int)g_mx_min;
  } else if (std::strcmp(key, "mx_seg_min") == 0) {
    *value = (int)g_mx_seg_min;
  } else if (std::strcmp(key, "mx_step") == 0) {
    *value = (int)std::lround(g_mx_step * 100.0);
  } else if (std::strcmp(key, "geom_tput") == 0) {
    *value = (int)std::lround(g_geom_tput * 100.0);
  } else if (std::strcmp(key, "geom_policy") == 0) {
    *value = g_geom_policy;
  } else if (std::strcmp(key, "sched_width") == 0) {
    *value = g_sched_width;
  } else if (std::strcmp(key, "fixed_window") == 0) {
    *value = g_fixed_win;
  } else if (std::strcmp(key, "fb_split") == 0) {
    *value = g_fb_split;
  } else if (std::strcmp(key, "lanes") == 0) {
    *value = g_lanes.load();
  } else if (std::strcmp(key, "ec_msm_ws_mb") == 0) {
    *value = g_ec_msm_ws_mb;
  } else {
    return fail(MPCX_EINVAL, "option %s cannot be read", key);
  }
  return MPCX_OK;
}

int mpcx_set_option(const char* key, int value) {
  if (!key) return fail(MPCX_EINVAL, "null option");
  std::lock_guard<std::mutex> lk(g_mu);
  if (std::strcmp(key, "force_geom") == 0) {
    if (value < -1 || value >= MPCX_NUM_GEOMS) return fail(MPCX_EINVAL, "force_geom %d out of range", value);
    g_force_geom = value;
  } else if (std::strcmp(key, "sched_width") == 0) {
    // cap on the sliding-window width of shared exponents; 0: Go's 4-bit fixed window
    if (value < 0 || value > MPCX_SCHED_MAX_WIDTH) return fail(MPCX_EINVAL, "sched_width %d out of range", value);
    g_sched_width = value;
  } else if (std::strcmp(key, "narrow_rounds") == 0) {
    // batches below value/100 of a resident round run in the narrow geometry
    if (value < 0 || value > 100) return fail(MPCX_EINVAL, "narrow_rounds %d out of range", value);
    g_narrow_rounds = value / 100.0;
  } else if (std::strcmp(key, "fb_window") == 0) {
    // window width of fixed-base tables registered from now on (4..12; one
    // product per window, 2^w entries per window)
    if (value < 4 || value > MPCX_FB_MAX_WINDOW_BITS) return fail(MPCX_EINVAL, "fb_window %d out of range", value);
    g_fb_window = value;
  } else if (std::strcmp(key, "fb_split") == 0) {
    // wavefronts sharing one comb operand's windows: 1, 2, 4; 0 picks by launch size
    if (value != 0 && value != 1 && value != 2 && value != 4) return fail(MPCX_EINVAL, "fb_split %d not 0/1/2/4", value);
    g_fb_split = value;
  } else if (std::strcmp(key, "mx") == 0) {
    // 1: batches of the 4096-bit main geometry reduce on the matrix cores (k_modexp_mx);
    // 2: the 2048-bit lane-pair geometry's as well
    if (value < 0 || value > 2) return fail(MPCX_EINVAL, "mx %d not 0, 1 or 2", value);
    g_mx = value;
  } else if (std::strcmp(key, "nsq") == 0) {
    // 1: a single k_modexp_mx batch with a shared exponent and a perfect-square modulus N^2
    // runs on N-adic pairs (k_modexp_nsq); 0: k_modexp_mx
    if (value < 0 || value > 1) return fail(MPCX_EINVAL, "nsq %d not 0 or 1", value);
    g_nsq = value;
  } else if (std::strcmp(key, "mx_min") == 0) {
    if (value < 1) return fail(MPCX_EINVAL, "mx_min %d < 1", value);
    g_mx_min = (uint32_t)value;
  } else if (std::strcmp(key, "mx_seg_min") == 0) {
    if (value < 1) return fail(MPCX_EINVAL, "mx_seg_min %d < 1", value);
    g_mx_seg_min = (uint32_t)value;
  } else if (std::strcmp(key, "mx_step") == 0) {
    // the launch-time model's k_modexp_mx wave-round time relative to k_modexp, x100 (100: as CIOS)
    if (value < 10 || value > 200) return fail(MPCX_EINVAL, "mx_step %d outside [10, 200]", value);
    g_mx_step = value / 100.0;
  } else if (std::strcmp(key, "geom_tput") == 0) {
    // the launch-time model's weight on the launch's share of the GPU's SIMD time, x100
    if (value < 0 || value > 1000) return fail(MPCX_EINVAL, "geom_tput %d outside [0, 1000]", value);
    g_geom_tput = value / 100.0;
  } else if (std::strcmp(key, "fixed_window") == 0) {
    // widest fixed window of per-operand exponents: 4 (Go's) or 5 (above 320 bits)
    if (value != 4 && value != 5) return fail(MPCX_EINVAL, "fixed_window %d not 4 or 5", value);
    g_fixed_win = value;
  } else if (std::strcmp(key, "lanes") == 0) {
    // execution lanes per device in use from now on (1..8; streams are created on first use)
    if (value < 1 || value > kMaxLanes) return fail(MPCX_EINVAL, "lanes %d outside [1, %d]", value, kMaxLanes);
    g_lanes = value;
  } else if (std::strcmp(key, "geom_policy") == 0) {
    // 1: the 4096-bit class picks main / mid / narrow by the launch-time model; 0: thresholds;
    // 2: the main geometry for every batch
    if (value < 0 || value > 2) return fail(MPCX_EINVAL, "geom_policy %d out of range", value);
    g_geom_policy = value;
  } else if (std::strcmp(key, "main_geom") == 0) {
    // main (throughput) geometry of the geometry's class
    if (value < 0 || value >= MPCX_NUM_GEOMS) return fail(MPCX_EINVAL, "main_geom %d out of range", value);
    g_main_geom[MPCX_GEOM_CLASS(value)] = value;
  } else if (std::strcmp(key, "duplicate_device") == 0) {
    // test hook: mpcx_init(ordinal) binds an already bound ordinal again as another logical device
    g_dup_device = value != 0;
  } else if (std::strcmp(key, "kernel_stats") == 0) {
    // time every batch-entry-point kernel with an event pair (mpcx_kernel_stats)
    g_kstats = value != 0;
  } else if (std::strcmp(key, "ec_msm_ws_mb") == 0) {
    // test hook: cap, in MB, on the table workspace of one k_ec_msm launch (at least one block runs)
    if (value < 1 || value > 4096) return fail(MPCX_EINVAL, "ec_msm_ws_mb %d outside [1, 4096]", value);
    g_ec_msm_ws_mb = value;
  } else if (std::strcmp(key, "device_split_min") == 0) {
    // smallest per-device slice of a host-buffer batch split across the bound GPUs (0: never split)
    if (value < 0) return fail(MPCX_EINVAL, "device_split_min %d < 0", value);
    g_split_min = (uint32_t)value;
  } else {
    return fail(MPCX_EINVAL, "unknown option %s", key);
  }
  return MPCX_OK;
}

const char* mpcx_last_error(void) { return g_err.c_str(); }

int mpcx_device_count(int* out_count) {
  if (!out_count) return fail(MPCX_EINVAL, "null out_count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *out_count = n;
  return MPCX_OK;
}

// launch-policy overrides from the environment (A/B runs of whole drivers)
static void read_env_options() {
  const char* nr = std::getenv("MPCX_NARROW_ROUNDS");  // percent of a main round
  if (nr) g_narrow_rounds = std::max(0, std::min(100, std::atoi(nr))) / 100.0;
  const char* gp = std::getenv("MPCX_GEOM_POLICY");
  if (gp) g_geom_policy = std::max(0, std::min(2, std::atoi(gp)));
  const char* ln = std::getenv("MPCX_LANES");
  if (ln && g_ndev.load() == 0) g_lanes = std::max(1, std::min(kMaxLanes, std::atoi(ln)));
  const char* fw = std::getenv("MPCX_FB_WINDOW");  // fixed-base comb width of new tables
  if (fw) g_fb_window = std::max(4, std::min(MPCX_FB_MAX_WINDOW_BITS, std::atoi(fw)));
  const char* mx = std::getenv("MPCX_MX");  // geometry-2 batches on k_modexp_mx
  if (mx) g_mx = std::max(0, std::min(2, std::atoi(mx)));
  const char* nq = std::getenv("MPCX_NSQ");  // N^2 batches with a shared exponent on k_modexp_nsq
  if (nq) g_nsq = std::max(0, std::min(1, std::atoi(nq)));
  const char* ms = std::getenv("MPCX_MX_STEP");  // x100, the launch-time model's k_modexp_mx step (A/B runs)
  if (ms) g_mx_step = std::max(10, std::min(200, std::atoi(ms))) / 100.0;
  const char* gt = std::getenv("MPCX_GEOM_TPUT");  // x100, the launch-time model's GPU-share weight
  if (gt) g_geom_tput = std::max(0, std::min(1000, std::atoi(gt))) / 100.0;
}

int mpcx_init(int device) {
  std::lock_guard<std::mutex> lk(g_mu);
  read_env_options();
  return bind_new_device(device);
}

int mpcx_init_devices(int n_gpus) {
  std::lock_guard<std::mutex> lk(g_mu);
  read_env_options();
  int vis = 0;
  hipError_t e = hipGetDeviceCount(&vis);
  if (e != hipSuccess || vis <= 0) return fail(MPCX_ENODEV, "no HIP device visible");
  if (n_gpus <= 0) n_gpus = vis;
  if (n_gpus > vis) return fail(MPCX_EINVAL, "%d GPUs requested, %d visible", n_gpus, vis);
  for (int i = 0; i < n_gpus; ++i)
    if (int rc = bind_new_device(i)) return rc;
  return MPCX_OK;
}

int mpcx_bound_devices(int* out_count, int* ordinals, int max_ordinals) {
  if (!out_count) return fail(MPCX_EINVAL, "null out_count");
  const int n = g_ndev.load(std::memory_order_acquire);
  *out_count = n;
  for (int i = 0; ordinals && i < n && i < max_ordinals; ++i) ordinals[i] = g_devs[i].ordinal;
  return MPCX_OK;
}

int mpcx_partition(uint32_t count, int n_devices, uint32_t min_slice, uint32_t* first, uint32_t* n,
                   uint32_t* n_slices) {
  if (!n_slices) return fail(MPCX_EINVAL, "null n_slices");
  if (n_devices < 1 || n_devices > kMaxDevices) return fail(MPCX_EINVAL, "n_devices %d outside [1, %d]", n_devices, kMaxDevices);
  *n_slices = partition(count, n_devices, min_slice, first, n);
  return MPCX_OK;
}

int mpcx_device_launches(int index, uint64_t* out) {
  const int n = g_ndev.load(std::memory_order_acquire);
  if (!out) return fail(MPCX_EINVAL, "null out");
  if (index < 0 || index >= n) return fail(MPCX_EINVAL, "device index %d not bound (%d bound)", index, n);
  *out = g_devs[index].launches.load();
  return MPCX_OK;
}

int mpcx_kernel_stats(char* buf, size_t cap, int reset) {
  const int n = g_ndev.load(std::memory_order_acquire);
  std::string out;
  {
    std::lock_guard<std::mutex> lk(g_kmu);
    double busy = 0.0, alg = 0.0;
    for (int i = 0; i < n && i < 8; ++i) {  // union of the device's kernel intervals
      auto iv = g_kiv[i];
      std::sort(iv.begin(), iv.end());
      double s0 = 0.0, e0 = -1.0;
      for (const auto& x : iv) {
        if (x.first > e0) {
          if (e0 > s0) busy += e0 - s0;
          s0 = x.first;
          e0 = x.second;
        } else {
          e0 = std::max(e0, x.second);
        }
      }
      if (e0 > s0) busy += e0 - s0;
    }
    char line[320];
    std::string ks;
    for (const auto& kv : g_kagg) {
      alg += kv.second.alg;
      std::snprintf(line, sizeof line,
                    "%s{\"kind\":\"%s\",\"geom\":%d,\"launches\":%llu,\"operands\":%llu,\"alg_macs\":%.6e,"
                    "\"kernel_ms\":%.4f,\"nsq_launches\":%llu}",
                    ks.empty() ? "" : ",", kv.first.first.c_str(), kv.first.second,
                    (unsigned long long)kv.second.launches, (unsigned long long)kv.second.ops, kv.second.alg,
                    kv.second.ms, (unsigned long long)kv.second.nsq);
      ks += line;
    }
    std::snprintf(line, sizeof line, "{\"enabled\":%d,\"busy_ms\":%.4f,\"alg_macs\":%.6e,\"kernels\":[",
                  g_kstats.load() ? 1 : 0, busy, alg);
    out = line + ks + "]}";
    if (reset) {
      g_kagg.clear();
      for (auto& v : g_kiv) v.clear();
    }
  }
  if (reset) {  // new time origin on every bound device
    for (int i = 0; i < n; ++i) {
      Device& d = g_devs[i];
      if (int rc = bind(d)) return rc;
      hipError_t e = d.kref ? hipSuccess : hipEventCreate(&d.kref);
      if (e == hipSuccess) e = hipEventRecord(d.kref, nullptr);
      if (e == hipSuccess) e = hipEventSynchronize(d.kref);
      if (e != hipSuccess) return hip_fail(e, "kernel stats time origin");
      if (i < 8) g_kref_host_ns[i] = mono_ns();
    }
  }
  if (buf && cap) {
    if (out.size() + 1 > cap) return fail(MPCX_EINVAL, "kernel stats need %zu bytes", out.size() + 1);
    std::memcpy(buf, out.c_str(), out.size() + 1);
  }
  return MPCX_OK;
}

int mpcx_select_device(int index) {
  const int n = g_ndev.load(std::memory_order_acquire);
  if (index < 0 || index >= n) return fail(MPCX_EINVAL, "device index %d not bound (%d bound)", index, n);
  t_sel = index;
  return bind(g_devs[index]);
}

int mpcx_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int n = g_ndev.load();
  for (int i = 0; i < n; ++i) {
    Device& d = g_devs[i];
    if (hipSetDevice(d.ordinal) != hipSuccess) continue;
    t_hip = d.ordinal;
    for (auto& l : d.lanes) drop_lane(l);
    drop_lane(d.build_lane);
    if (d.ec_gtab) (void)hipFree(d.ec_gtab);
    d.ec_gtab = nullptr;
    if (d.ed_btab) (void)hipFree(d.ed_btab);
    d.ed_btab = nullptr;
    {
      std::lock_guard<std::mutex> dl(d.dev_mu);
      for (auto& kv : d.dev_lanes) drop_lane(*kv.second);
      d.dev_lanes.clear();
    }
    d.ordinal = -1;
  }
  g_stage_chunks.release_all();
  free_retired();
  g_ndev.store(0);
  return MPCX_OK;
}

int mpcx_modulus_register(const uint32_t* m_words, uint32_t m_len, mpcx_mod_t* out) {
  if (!m_words || !out || m_len == 0) return fail(MPCX_EINVAL, "null modulus or output");
  Device* dev = nullptr;
  if (int rc = selected(&dev)) return rc;
  std::vector<uint32_t> m(m_words, m_words + m_len);
  while (m.size() > 1 && m.back() == 0) m.pop_back();
  const uint32_t bits = bit_length(m);
  if (bits == 0) return fail(MPCX_EINVAL, "modulus is zero");
  if ((m[0] & 1u) == 0) return fail(MPCX_EINVAL, "modulus is even (math/big uses a non-Montgomery path; keep it on the host)");
  const int cls = class_for_bits(bits);
  if (cls < 0) return fail(MPCX_EINVAL, "modulus has %u bits > %d", bits, MPCX_MAX_MODULUS_BITS);
  auto* mod = new mpcx_modulus_s();
  mod->cls = cls;
  mod->bits = bits;
  mod->words = (uint32_t)m.size();
  mod->m = m;
  uint32_t inv = m[0];
  for (int i = 0; i < 5; ++i) inv *= 2u - m[0] * inv;
  mod->n0inv = (0u - inv) & kM28;
  for (int g = 0; g < MPCX_NUM_GEOMS; ++g) {
    mod->const_off[g] = 0;
    if (MPCX_GEOM_CLASS(g) != cls) continue;
    const uint32_t L = (uint32_t)MPCX_GEOM_L(g);
    mod->const_off[g] = (uint32_t)mod->host_const.size();
    auto nd = to_digits(m, L);
    auto r1 = to_digits(pow2_mod(kDigitBits * L, m), L);
    auto r2 = to_digits(pow2_mod(2 * kDigitBits * L, m), L);
    auto& h = mod->host_const;
    h.insert(h.end(), nd.begin(), nd.end());
    h.insert(h.end(), r1.begin(), r1.end());
    h.insert(h.end(), r2.begin(), r2.end());
  }
  // upload to the selected device now (fails loudly without memory); other
  // bound devices receive the constants on first use
  const uint32_t* p = nullptr;
  if (int rc = mod_const(mod, (int)(dev - g_devs), &p)) {
    delete mod;
    return rc;
  }
  *out = mod;
  return MPCX_OK;
}

int mpcx_modulus_release(mpcx_mod_t mod) {
  if (!mod) return fail(MPCX_EINVAL, "null modulus");
  const int n = g_ndev.load();
  for (int i = 0; i < n && i < kMaxDevices; ++i) {
    if (mod->d_const[i] && bind(g_devs[i]) == MPCX_OK) (void)hipFree(mod->d_const[i]);
    if (mod->d_mx[i] && bind(g_devs[i]) == MPCX_OK) (void)hipFree(mod->d_mx[i]);
    if (mod->d_nsq[i] && bind(g_devs[i]) == MPCX_OK) (void)hipFree(mod->d_nsq[i]);
  }
  delete mod;
  return MPCX_OK;
}

int mpcx_mx_tables(const uint32_t* m_words, uint32_t m_len, uint32_t L, uint8_t* out, size_t cap) {
  if (!m_words || !out || m_len == 0) return fail(MPCX_EINVAL, "null modulus or output");
  MxDims dm{};
  if (!mx_dims(L, &dm)) return fail(MPCX_EINVAL, "L %u is not an MX geometry's (148, 76 or 74)", L);
  if (cap < dm.img) return fail(MPCX_EINVAL, "mx tables need %u bytes", dm.img);
  std::vector<uint32_t> m(m_words, m_words + m_len);
  while (m.size() > 1 && m.back() == 0) m.pop_back();
  // R = 2^(28 L) > 4m
  if ((m[0] & 1u) == 0 || bit_length(m) + 2 > kDigitBits * L)
    return fail(MPCX_EINVAL, "mx tables need an odd modulus of < %u bits", kDigitBits * L - 2);
  std::vector<uint8_t> t;
  mx_tables(m, L, t);
  std::memcpy(out, t.data(), dm.img);
  return MPCX_OK;
}

int mpcx_nsq_consts(const uint32_t* m_words, uint32_t m_len, uint32_t* out, size_t cap_words, int* is_square) {
  if (!m_words || !is_square || m_len == 0) return fail(MPCX_EINVAL, "null modulus or output");
  std::vector<uint32_t> m(m_words, m_words + m_len);
  while (m.size() > 1 && m.back() == 0) m.pop_back();
  if ((m[0] & 1u) == 0 || class_for_bits(bit_length(m)) != 2)
    return fail(MPCX_EINVAL, "nsq constants need an odd modulus of the 4096-bit class");
  std::vector<uint32_t> c;
  *is_square = nsq_build(m, c) ? 1 : 0;
  if (*is_square) {
    if (!out || cap_words < c.size()) return fail(MPCX_EINVAL, "nsq constants need %zu words", c.size());
    std::memcpy(out, c.data(), c.size() * sizeof(uint32_t));
  }
  return MPCX_OK;
}

int mpcx_modulus_info(mpcx_mod_t mod, uint32_t* out_bits, uint32_t* out_class_words) {
  if (!mod) return fail(MPCX_EINVAL, "null modulus");
  if (out_bits) *out_bits = mod->bits;
  if (out_class_words) *out_class_words = (uint32_t)MPCX_CLASS_WORDS(mod->cls);
  return MPCX_OK;
}

int mpcx_modulus_geometry(mpcx_mod_t mod, uint32_t* L, uint32_t* P, uint32_t* K, uint32_t* G) {
  if (!mod) return fail(MPCX_EINVAL, "null modulus");
  const int g = main_geom_for(mod, true);
  if (L) *L = (uint32_t)MPCX_GEOM_L(g);
  if (P) *P = (uint32_t)MPCX_GEOM_P(g);
  if (K) *K = (uint32_t)MPCX_GEOM_K(g);
  if (G) *G = (uint32_t)MPCX_GEOM_G(g);
  return MPCX_OK;
}

}  // extern "C"

// Enqueue one batch on lane `lane` of device `di` (lane locked by the caller;
// its stream is lane.st).
// ops_fit: every base and multiplier is below 2^MPCX_GEOM_RBITS of the class's
// main geometry (host_ops_below; see geom_serves). alg_macs: the batch's
// Go-equivalent MACs where the host has the operands' own exponents (< 0: from
// exp_bits).
static int modexp_enqueue(int di, Lane& lane, mpcx_mod_t mod, uint32_t count, const uint32_t* d_bases,
                          uint32_t base_words, const uint32_t* d_exps, uint32_t exp_words, int exp_shared,
                          uint32_t exp_bits, const uint32_t* d_muls, uint32_t mul_words, uint32_t* d_out,
                          uint32_t out_words, bool ops_fit, double alg_macs = -1.0) {
  Device& dev = g_devs[di];
  int rc;
  if ((rc = check_batch("", mod, count, d_bases, base_words, d_exps, exp_words, d_muls, mul_words, d_out, out_words)))
    return rc;
  if (exp_bits > 32u * exp_words) return fail(MPCX_EINVAL, "exp_bits %u > 32*exp_words", exp_bits);
  if (count == 0) return MPCX_OK;
  const uint32_t* dconst = nullptr;
  if ((rc = mod_const(mod, di, &dconst))) return rc;
  const int cls = mod->cls;
  // a forced geometry is tested with the caller's ops_fit, which was computed
  // against the main geometry's R (mpcx_modexp_multi_batch rescans the operands
  // against the forced geometry's)
  const bool forced_serves =
      g_force_geom >= 0 && MPCX_GEOM_CLASS(g_force_geom) == cls && geom_serves(g_force_geom, mod, ops_fit);
  // the model's mx input asks about the main geometry this batch would get, the
  // full-width one where the configured main cannot serve it (the multi path
  // asks about the class's default main geometry)
  const int gmain = main_geom_for(mod, ops_fit);
  const bool mx_ok = runs_on_mx(gmain, count, count, false) && mx_serves(gmain, mod);
  const int geom = choose_geom(dev, cls, count, geom_serves(g_main_geom[cls], mod, ops_fit), forced_serves, mx_ok);
  const uint32_t G = (uint32_t)MPCX_GEOM_G(geom), K = (uint32_t)MPCX_GEOM_K(geom);
  const uint32_t waves = (count + G - 1) / G;
  // a shared exponent's sliding-window schedule lives after the tables
  const bool use_sched = exp_shared && exp_bits > 0 && g_sched_width > 0;
  const bool mx = runs_on_mx(geom, count, count, false) && mx_serves(geom, mod);
  // m = N^2 with a shared exponent and no multiplier: k_modexp_nsq (N-adic pairs,
  // the same wavefront split as geometry 2) in place of k_modexp_mx
  const uint32_t* dnsq = nullptr;
  if (g_nsq && mx && geom == 2 && use_sched && !d_muls && (rc = nsq_const(mod, di, &dnsq))) return rc;
  const size_t sched_off = (size_t)waves * MPCX_TABLE_ENTRIES * (dnsq ? (uint32_t)MPCX_NSQ_TABLE_SLOTS : K) * 64u;
  const size_t ws_words = sched_off + (use_sched ? MPCX_SCHED_WORDS(32u * exp_words) : 0);
  if ((rc = ensure_workspace(lane, ws_words * sizeof(uint32_t)))) return rc;
  uint32_t* sched = use_sched ? lane.ws + sched_off : nullptr;
  if (use_sched && (rc = launch_expsched(d_exps, exp_words, sched, lane.st))) return rc;
  const uint8_t* mx_img = nullptr;
  if (dnsq) {
    mx_img = reinterpret_cast<const uint8_t*>(dnsq + MPCX_NSQ_CONST_DIGITS);
  } else if (mx && (rc = mx_const(mod, di, &mx_img))) {
    return rc;
  }
  mpcx::ModexpArgs a =
      modexp_args(mod, geom, dconst, count, d_bases, base_words, d_exps, exp_words, d_muls, mul_words, d_out,
                  out_words, lane.ws, exp_bits, exp_shared, sched, mx_img, waves);
  a.nsq = dnsq;
  const char* kind = mx ? "modexp_mx" : "modexp";
  const int ks = kstat_begin(lane);
  hipError_t e = mpcx_launch_modexp(geom, &a, waves, lane.st);
  if (e != hipSuccess) return hip_fail(e, "launch k_modexp");
  dev.launches.fetch_add(1, std::memory_order_relaxed);
  const double alg = alg_macs >= 0 ? alg_macs : go_macs(mod->bits, a.exp_bits) * count;
  // k_modexp_nsq stays under the kind of the kernel it stands in for (the plans and
  // rooflines read "modexp_mx"); the entry's nsq_launches tells the two apart
  kstat_end(lane, ks, dev, di, kind, geom, count, alg, dnsq != nullptr);
  launch_log(kind, geom, count, mod->bits, a.exp_bits, alg);
  return MPCX_OK;
}

static uint32_t max_exp_bits(const uint32_t* exps, uint32_t exp_words, int exp_shared, uint32_t count) {
  uint32_t bits = 0;
  if (!exp_words) return 0;
  if (exp_shared) return bit_length_words(exps, exp_words);
  for (uint32_t i = 0; i < count; ++i) bits = std::max(bits, bit_length_words(exps + (size_t)i * exp_words, exp_words));
  return bits;
}

// host-buffer path: stage one operand range on one device, launch, copy back (synchronous)
static int modexp_host_range(int di, mpcx_mod_t mod, uint32_t count, const uint32_t* bases, uint32_t base_words,
                             const uint32_t* exps, uint32_t exp_words, int exp_shared, const uint32_t* muls,
                             uint32_t mul_words, uint32_t* out, uint32_t out_words) {
  const uint32_t exp_bits = max_exp_bits(exps, exp_words, exp_shared, count);
  const size_t n_exp_words = exp_shared ? exp_words : (size_t)count * exp_words;
  const size_t bb = (size_t)count * base_words * 4, eb = std::max<size_t>(n_exp_words * 4, 4),
               ob = (size_t)count * out_words * 4, mb = muls ? (size_t)count * mul_words * 4 : 0;
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(g_devs[di], lk);
  LaneDrain drain(l);
  int rc;
  if ((rc = lane_stream(l))) return rc;
  Staging* sg = l.stage;
  if ((rc = ensure_buffer(sg[0], bb)) || (rc = ensure_buffer(sg[1], eb)) || (rc = ensure_buffer(sg[2], ob)) ||
      (muls && (rc = ensure_buffer(sg[3], mb))))
    return rc;
  if ((rc = h2d(l, sg[0].ptr, bases, bb)) || (rc = h2d(l, sg[1].ptr, exps, n_exp_words * 4)) ||
      (muls && (rc = h2d(l, sg[3].ptr, muls, mb))))
    return rc;
  const uint32_t rb = (uint32_t)MPCX_GEOM_RBITS(g_main_geom[mod->cls]);
  const bool ops_fit = host_ops_below(bases, count, base_words, rb) && host_ops_below(muls, count, mul_words, rb);
  // the operands' own exponent lengths (launch log)
  const double alg = !exp_shared && exp_words ? go_macs_sum(mod->bits, exps, exp_words, count) : -1.0;
  rc = modexp_enqueue(di, l, mod, count, (const uint32_t*)sg[0].ptr, base_words, (const uint32_t*)sg[1].ptr,
                      exp_words, exp_shared, exp_bits, muls ? (const uint32_t*)sg[3].ptr : nullptr, mul_words,
                      (uint32_t*)sg[2].ptr, out_words, ops_fit, alg);
  if (rc) return rc;
  return d2h_sync(out, sg[2].ptr, ob, l);
}

static int modexp_host(mpcx_mod_t mod, uint32_t count, const uint32_t* bases, uint32_t base_words,
                       const uint32_t* exps, uint32_t exp_words, int exp_shared, const uint32_t* muls,
                       uint32_t mul_words, uint32_t* out, uint32_t out_words) {
  if (!mod) return fail(MPCX_EINVAL, "null modulus");
  if (count == 0) return MPCX_OK;
  if (!bases || !out || (exp_words && !exps)) return fail(MPCX_EINVAL, "null buffer");
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t n) {
    return modexp_host_range(di, mod, n, bases + (size_t)first * base_words, base_words,
                             exps ? (exp_shared ? exps : exps + (size_t)first * exp_words) : nullptr, exp_words,
                             exp_shared, muls ? muls + (size_t)first * mul_words : nullptr, mul_words,
                             out + (size_t)first * out_words, out_words);
  });
}

// ------------------------------------------------------------ async jobs
// mpcx_modexp_submit: a host-buffer batch run by a small pool of submission
// threads, so a batcher (the Go side's one goroutine per modulus,
// INTEGRATION.md) can stage batch k+1 while batch k runs.
struct mpcx_job_s {
  std::mutex mu;
  std::condition_variable cv;
  bool done = false;
  int rc = MPCX_OK;
  std::string msg;
  std::function<int()> work;
};

namespace {
struct JobPool {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<mpcx_job_t> q;
  std::vector<std::thread> th;
  void start(size_t n) {
    while (th.size() < n)
      th.emplace_back([this] {
        for (;;) {
          mpcx_job_t j;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !q.empty(); });
            j = q.front();
            q.pop_front();
          }
          const int rc = j->work();
          std::lock_guard<std::mutex> lk(j->mu);
          j->rc = rc;
          if (rc) j->msg = g_err;
          j->done = true;
          j->cv.notify_all();
        }
      });
  }
};
JobPool& job_pool() {
  // never destroyed: worker threads live for the process
  static JobPool* p = new JobPool();
  return *p;
}
}  // namespace

extern "C" {

int mpcx_modexp_batch_device(mpcx_mod_t mod, uint32_t count, const uint32_t* d_bases, uint32_t base_words,
                             const uint32_t* d_exps, uint32_t exp_words, int exp_shared, uint32_t exp_bits,
                             uint32_t* d_out, uint32_t out_words, void* stream) {
  if (!mod) return fail(MPCX_EINVAL, "null modulus");
  Device* dev = nullptr;
  if (int rc = selected(&dev)) return rc;
  Lane& l = stream_lane(*dev, (hipStream_t)stream);
  std::lock_guard<std::mutex> lk(l.mu);
  // device buffers are not scanned: operands fit when their width does
  const bool ops_fit = 32u * base_words <= (uint32_t)MPCX_GEOM_RBITS(g_main_geom[mod->cls]);
  return modexp_enqueue((int)(dev - g_devs), l, mod, count, d_bases, base_words, d_exps, exp_words, exp_shared,
                        exp_bits, nullptr, 0, d_out, out_words, ops_fit);
}

int mpcx_modexp_mul_batch_device(mpcx_mod_t mod, uint32_t count, const uint32_t* d_bases, uint32_t base_words,
                                 const uint32_t* d_exps, uint32_t exp_words, int exp_shared, uint32_t exp_bits,
                                 const uint32_t* d_muls, uint32_t mul_words, uint32_t* d_out, uint32_t out_words,
                                 void* stream) {
  if (!mod) return fail(MPCX_EINVAL, "null modulus");
  if (!d_muls) return fail(MPCX_EINVAL, "null multipliers");
  Device* dev = nullptr;
  if (int rc = selected(&dev)) return rc;
  Lane& l = stream_lane(*dev, (hipStream_t)stream);
  std::lock_guard<std::mutex> lk(l.mu);
  const uint32_t rb = (uint32_t)MPCX_GEOM_RBITS(g_main_geom[mod->cls]);
  const bool ops_fit = 32u * base_words <= rb && 32u * mul_words <= rb;
  return modexp_enqueue((int)(dev - g_devs), l, mod, count, d_bases, base_words, d_exps, exp_words, exp_shared,
                        exp_bits, d_muls, mul_words, d_out, out_words, ops_fit);
}

int mpcx_modexp_batch(mpcx_mod_t mod, uint32_t count, const uint32_t* bases, uint32_t base_words,
                      const uint32_t* exps, uint32_t exp_words, int exp_shared, uint32_t* out,
                      uint32_t out_words) {
  return modexp_host(mod, count, bases, base_words, exps, exp_words, exp_shared, nullptr, 0, out, out_words);
}

int mpcx_modexp_mul_batch(mpcx_mod_t mod, uint32_t count, const uint32_t* bases, uint32_t base_words,
                          const uint32_t* exps, uint32_t exp_words, int exp_shared, const uint32_t* muls,
                          uint32_t mul_words, uint32_t* out, uint32_t out_words) {
  if (!muls) return fail(MPCX_EINVAL, "null multipliers");
  return modexp_host(mod, count, bases, base_words, exps, exp_words, exp_shared, muls, mul_words, out, out_words);
}

int mpcx_modexp_submit(mpcx_mod_t mod, uint32_t count, const uint32_t* bases, uint32_t base_words,
                       const uint32_t* exps, uint32_t exp_words, int exp_shared, const uint32_t* muls,
                       uint32_t mul_words, uint32_t* out, uint32_t out_words, mpcx_job_t* job) {
  if (!job) return fail(MPCX_EINVAL, "null job");
  *job = nullptr;
  if (!mod) return fail(MPCX_EINVAL, "null modulus");
  const int n = ndev_or_fail();
  if (n < 0) return -n;
  auto* j = new mpcx_job_s();
  j->work = [=] {
    return modexp_host(mod, count, bases, base_words, exps, exp_words, exp_shared, muls, mul_words, out, out_words);
  };
  JobPool& p = job_pool();
  {
    std::lock_guard<std::mutex> lk(p.mu);
    p.start((size_t)n * kMaxLanes);
    p.q.push_back(j);
  }
  p.cv.notify_one();
  *job = j;
  return MPCX_OK;
}

int mpcx_job_test(mpcx_job_t job, int* done) {
  if (!job || !done) return fail(MPCX_EINVAL, "null job");
  std::lock_guard<std::mutex> lk(job->mu);
  *done = job->done ? 1 : 0;
  return MPCX_OK;
}

int mpcx_job_wait(mpcx_job_t job) {
  if (!job) return fail(MPCX_EINVAL, "null job");
  int rc;
  {
    std::unique_lock<std::mutex> lk(job->mu);
    job->cv.wait(lk, [&] { return job->done; });
    rc = job->rc;
    if (rc) g_err = job->msg;
  }
  delete job;
  return rc;
}

int mpcx_mulmod_batch(mpcx_mod_t mod, uint32_t count, const uint32_t* a, uint32_t a_words, const uint32_t* b,
                      uint32_t b_words, uint32_t* out, uint32_t out_words) {
  if (!a || !b) return fail(MPCX_EINVAL, "null operands");
  const uint32_t one = 1;
  return modexp_host(mod, count, a, a_words, &one, 1, 1, b, b_words, out, out_words);
}

// ------------------------------------------------------------ multi-batch
// Several batches (moduli of one class) in one k_modexp_multi launch on one
// device: inputs packed into one staging buffer, per-group schedules, one
// segment table, one output copy scattered back to the groups.
int mpcx_modexp_multi_batch(uint32_t n_groups, const mpcx_modexp_group_t* gs) {
  if (n_groups == 0) return MPCX_OK;
  if (!gs) return fail(MPCX_EINVAL, "null groups");
  const int n = ndev_or_fail();
  if (n < 0) return -n;
  int cls = -1, rc;
  uint64_t total = 0;
  uint32_t min_seg = 0xFFFFFFFFu;  // the smallest non-empty group
  for (uint32_t i = 0; i < n_groups; ++i) {
    const mpcx_modexp_group_t& g = gs[i];
    if (!g.mod) return fail(MPCX_EINVAL, "group %u: null modulus", i);
    if (cls < 0) cls = g.mod->cls;
    if (g.mod->cls != cls) return fail(MPCX_EINVAL, "group %u: modulus class differs from group 0's", i);
    if (g.count == 0) continue;  // an empty group is not checked
    char pre[24];
    std::snprintf(pre, sizeof pre, "group %u: ", i);
    if ((rc = check_batch(pre, g.mod, g.count, g.bases, g.base_words, g.exps, g.exp_words, g.muls, g.mul_words, g.out,
                          g.out_words)))
      return rc;
    total += g.count;
    min_seg = std::min(min_seg, g.count);
  }
  if (total == 0) return MPCX_OK;
  if (total > 0xFFFFFFFFull) return fail(MPCX_EINVAL, "too many operands");
  const int di = (int)(g_dev_rr.fetch_add(1, std::memory_order_relaxed) % (unsigned)n);
  Device& dev = g_devs[di];
  if ((rc = bind(dev))) return rc;
  // every segment's modulus and operands fit the geometry; a forced geometry is
  // tested with the operands rescanned against its own R (modexp_enqueue tests it
  // with the scan against the main geometry's)
  bool main_ok = true, forced_ok = true;
  {
    const int gf = g_force_geom >= 0 && MPCX_GEOM_CLASS(g_force_geom) == cls ? g_force_geom : -1;
    const uint32_t rb = (uint32_t)MPCX_GEOM_RBITS(g_main_geom[cls]);
    for (uint32_t i = 0; i < n_groups && (main_ok || forced_ok); ++i) {
      const mpcx_modexp_group_t& g = gs[i];
      if (g.count == 0) continue;
      const bool fit = host_ops_below(g.bases, g.count, g.base_words, rb) &&
                       host_ops_below(g.muls, g.count, g.mul_words, rb);
      main_ok = main_ok && geom_serves(g_main_geom[cls], g.mod, fit);
      if (gf >= 0) {
        const uint32_t rf = (uint32_t)MPCX_GEOM_RBITS(gf);
        forced_ok = forced_ok && geom_serves(gf, g.mod, host_ops_below(g.bases, g.count, g.base_words, rf) &&
                                                            host_ops_below(g.muls, g.count, g.mul_words, rf));
      }
    }
  }
  // the model's mx input asks about the class's default main geometry (modexp_enqueue
  // asks about the main geometry its batch would get)
  const bool mx_ok = runs_on_mx(MPCX_MAIN_GEOM(cls), (uint32_t)total, min_seg, true);
  const int geom = choose_geom(dev, cls, (uint32_t)total, main_ok, forced_ok, mx_ok);
  const uint32_t G = (uint32_t)MPCX_GEOM_G(geom), K = (uint32_t)MPCX_GEOM_K(geom);
  // (geometry 2 only: every modulus of its class passes mx_serves)
  const bool mx = runs_on_mx(geom, (uint32_t)total, min_seg, true);
  // host-side layout of the packed inputs and outputs (words)
  struct Seg {
    uint32_t gi, waves, exp_bits;
    size_t in_b, in_e, in_m, out_o, ws, sched;
    bool use_sched;
    double alg;
  };
  std::vector<Seg> segs;
  size_t in_words = 0, out_words = 0, ws_words = 0;
  for (uint32_t i = 0; i < n_groups; ++i) {
    const mpcx_modexp_group_t& g = gs[i];
    if (g.count == 0) continue;
    Seg sg{};
    sg.gi = i;
    sg.waves = (g.count + G - 1) / G;
    sg.exp_bits = max_exp_bits(g.exps, g.exp_words, g.exp_shared, g.count);
    sg.in_b = in_words;
    in_words += (size_t)g.count * g.base_words;
    sg.in_e = in_words;
    in_words += g.exp_shared ? g.exp_words : (size_t)g.count * g.exp_words;
    sg.in_m = in_words;
    if (g.muls) in_words += (size_t)g.count * g.mul_words;
    sg.out_o = out_words;
    out_words += (size_t)g.count * g.out_words;
    sg.ws = ws_words;
    ws_words += (size_t)sg.waves * MPCX_TABLE_ENTRIES * K * 64u;
    sg.use_sched = g.exp_shared && sg.exp_bits > 0 && g_sched_width > 0;
    sg.alg = g.exp_shared || !g.exp_words ? go_macs(g.mod->bits, sg.exp_bits) * g.count
                                          : go_macs_sum(g.mod->bits, g.exps, g.exp_words, g.count);
    segs.push_back(sg);
  }
  for (auto& sg : segs)
    if (sg.use_sched) {
      sg.sched = ws_words;
      ws_words += MPCX_SCHED_WORDS(32u * gs[sg.gi].exp_words);
    }
  const size_t nseg = segs.size();
  const size_t seg_bytes = nseg * sizeof(mpcx::ModexpArgs), first_bytes = (nseg + 1) * sizeof(uint32_t);
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(dev, lk);
  LaneDrain drain(l);
  if ((rc = lane_stream(l))) return rc;
  if ((rc = ensure_buffer(l.stage[0], std::max<size_t>(in_words * 4, 4))) ||
      (rc = ensure_buffer(l.stage[2], out_words * 4)) || (rc = ensure_buffer(l.stage[3], seg_bytes + first_bytes)) ||
      (rc = ensure_workspace(l, ws_words * 4)))
    return rc;
  const uint32_t* d_in = (const uint32_t*)l.stage[0].ptr;
  uint32_t* d_out = (uint32_t*)l.stage[2].ptr;
  // each group's arrays straight from the caller's buffers into their offsets
  // (DMA from page-locked buffers such as libmpcx_host's; no host-side packing)
  for (const auto& sg : segs) {
    const mpcx_modexp_group_t& g = gs[sg.gi];
    const size_t ne = g.exp_shared ? g.exp_words : (size_t)g.count * g.exp_words;
    if ((rc = h2d(l, (uint32_t*)l.stage[0].ptr + sg.in_b, g.bases, (size_t)g.count * g.base_words * 4)) ||
        (rc = h2d(l, (uint32_t*)l.stage[0].ptr + sg.in_e, g.exps, ne * 4)) ||
        (g.muls && (rc = h2d(l, (uint32_t*)l.stage[0].ptr + sg.in_m, g.muls, (size_t)g.count * g.mul_words * 4))))
      return rc;
  }
  std::vector<mpcx::ModexpArgs> args(nseg);
  std::vector<uint32_t> first(nseg + 1, 0);
  for (size_t k = 0; k < nseg; ++k) {
    const Seg& sg = segs[k];
    const mpcx_modexp_group_t& g = gs[sg.gi];
    const uint32_t* dconst = nullptr;
    const uint8_t* mx_img = nullptr;
    if ((rc = mod_const(g.mod, di, &dconst)) || (mx && (rc = mx_const(g.mod, di, &mx_img)))) return rc;
    uint32_t* sched = sg.use_sched ? l.ws + sg.sched : nullptr;
    if (sg.use_sched && (rc = launch_expsched(d_in + sg.in_e, g.exp_words, sched, l.st))) return rc;
    args[k] = modexp_args(g.mod, geom, dconst, g.count, d_in + sg.in_b, g.base_words,
                          g.exp_words ? d_in + sg.in_e : nullptr, g.exp_words, g.muls ? d_in + sg.in_m : nullptr,
                          g.mul_words, d_out + sg.out_o, g.out_words, l.ws + sg.ws, sg.exp_bits, g.exp_shared, sched,
                          mx_img, sg.waves);
    // mx: each segment starts on a workgroup of MX_WG wavefronts (first[] counts workgroups)
    first[k + 1] = first[k] + (mx ? (sg.waves + MX_WG - 1) / MX_WG : sg.waves);
  }
  if ((rc = h2d(l, l.stage[3].ptr, args.data(), seg_bytes)) ||
      (rc = h2d(l, (char*)l.stage[3].ptr + seg_bytes, first.data(), first_bytes)))
    return rc;
  const int ks = kstat_begin(l);
  hipError_t e = mpcx_launch_modexp_multi(geom, (const mpcx::ModexpArgs*)l.stage[3].ptr,
                                          (const uint32_t*)((const char*)l.stage[3].ptr + seg_bytes),
                                          (uint32_t)nseg, first[nseg], mx ? 1 : 0, l.st);
  if (e != hipSuccess) return hip_fail(e, "launch k_modexp_multi");
  dev.launches.fetch_add(1, std::memory_order_relaxed);
  const char* kind = mx ? "modexp_multi_mx" : "modexp_multi";
  double alg = 0.0;
  for (const auto& sg : segs) alg += sg.alg;
  kstat_end(l, ks, dev, di, kind, geom, (uint32_t)total, alg);
  for (const auto& sg : segs) launch_log(kind, geom, gs[sg.gi].count, gs[sg.gi].mod->bits, sg.exp_bits, sg.alg);
  for (const auto& sg : segs) {  // results straight into each group's buffer
    const mpcx_modexp_group_t& g = gs[sg.gi];
    if ((rc = d2h(l, g.out, d_out + sg.out_o, (size_t)g.count * g.out_words * 4))) return rc;
  }
  return lane_wait(l);
}

// ------------------------------------------------------------ secp256k1
namespace {
constexpr uint32_t kEcG[16] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu, 0xCE870B07u, 0x55A06295u,
                               0xF9DCBBACu, 0x79BE667Eu, 0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u,
                               0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};
constexpr uint32_t kEcTabEntries = 32u * 255u;
constexpr size_t ec_ws_words(uint32_t count) { return (size_t)((count + 63u) / 64u) * 30u * 24u * 64u; }

// The base-point comb of device d (built on first use by k_ec_combine itself:
// entry (w, v) = (v 2^(8w)) G as a plain scalar multiple of G). Lane l locked.
int ec_gtab(Device& d, Lane& l, const uint32_t** out) {
  std::lock_guard<std::mutex> lk(d.ec_mu);
  if (!d.ec_gtab) {
    std::vector<uint32_t> sc((size_t)kEcTabEntries * 24u, 0u), pts((size_t)kEcTabEntries * 32u, 0u);
    for (uint32_t w = 0; w < 32; ++w)
      for (uint32_t v = 1; v <= 255; ++v) {
        const size_t e = (size_t)w * 255u + (v - 1u);
        const uint32_t bit = 8u * w;  // b = v << bit (spans at most two words)
        const uint64_t x = (uint64_t)v << (bit % 32u);
        sc[e * 24u + 8u + bit / 32u] = (uint32_t)x;
        if (bit / 32u + 1u < 8u) sc[e * 24u + 8u + bit / 32u + 1u] = (uint32_t)(x >> 32);
        std::memcpy(&pts[e * 32u], kEcG, sizeof kEcG);
      }
    int rc;
    const size_t sb = sc.size() * 4, pb = pts.size() * 4;
    if ((rc = ensure_buffer(l.stage[0], sb)) || (rc = ensure_buffer(l.stage[1], pb)) ||
        (rc = ensure_workspace(l, ec_ws_words(kEcTabEntries) * 4)))
      return rc;
    uint32_t* tab = nullptr;
    hipError_t e = hipMalloc((void**)&tab, (size_t)kEcTabEntries * 16u * 4u);
    if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(secp256k1 comb): %s", hipGetErrorString(e));
    if ((rc = h2d(l, l.stage[0].ptr, sc.data(), sb)) || (rc = h2d(l, l.stage[1].ptr, pts.data(), pb))) {
      (void)hipFree(tab);
      return rc;
    }
    e = mpcx_launch_ec_combine((const uint32_t*)l.stage[0].ptr, (const uint32_t*)l.stage[1].ptr, tab, nullptr, l.ws,
                               kEcTabEntries, l.st);
    if (e != hipSuccess) {
      (void)hipFree(tab);
      return hip_fail(e, "launch k_ec_combine (comb build)");
    }
    if ((rc = lane_wait(l))) {
      (void)hipFree(tab);
      return rc;
    }
    d.ec_gtab = tab;
  }
  *out = d.ec_gtab;
  return MPCX_OK;
}

int ec_range(int di, uint32_t count, const uint32_t* scalars, const uint32_t* points, uint32_t* out) {
  Device& d = g_devs[di];
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(d, lk);
  LaneDrain drain(l);
  int rc;
  if ((rc = lane_stream(l))) return rc;
  const uint32_t* gtab = nullptr;
  if ((rc = ec_gtab(d, l, &gtab))) return rc;
  const size_t sb = (size_t)count * 24u * 4u, pb = (size_t)count * 32u * 4u, ob = (size_t)count * 16u * 4u;
  if ((rc = ensure_buffer(l.stage[0], sb)) || (rc = ensure_buffer(l.stage[1], pb)) ||
      (rc = ensure_buffer(l.stage[2], ob)) || (rc = ensure_workspace(l, ec_ws_words(count) * 4)))
    return rc;
  if ((rc = h2d(l, l.stage[0].ptr, scalars, sb)) || (rc = h2d(l, l.stage[1].ptr, points, pb))) return rc;
  const int ks = kstat_begin(l);
  hipError_t e = mpcx_launch_ec_combine((const uint32_t*)l.stage[0].ptr, (const uint32_t*)l.stage[1].ptr,
                                        (uint32_t*)l.stage[2].ptr, gtab, l.ws, count, l.st);
  if (e != hipSuccess) return hip_fail(e, "launch k_ec_combine");
  kstat_end(l, ks, d, di, "ec_combine", -1, count, 0.0);
  d.launches.fetch_add(1, std::memory_order_relaxed);
  launch_log("ec_combine", -1, count, 256, 256, 0.0);
  return d2h_sync(out, l.stage[2].ptr, ob, l);
}
}  // namespace

int mpcx_ec_combine_batch(uint32_t count, const uint32_t* scalars, const uint32_t* points, uint32_t* out) {
  if (count == 0) return MPCX_OK;
  if (!scalars || !points || !out) return fail(MPCX_EINVAL, "null buffer");
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t n) {
    return ec_range(di, n, scalars + (size_t)first * 24u, points + (size_t)first * 32u, out + (size_t)first * 16u);
  });
}

namespace {
// k_ec_msm's per-thread tables: 15 Jacobian entries of 24 words per point, 64 lanes per block
constexpr size_t kEcMsmPointBytes = 15u * 24u * 64u * 4u;

int ec_msm_range(int di, uint32_t count, uint32_t n_points, const uint32_t* a, const uint32_t* scalars,
                 const uint32_t* points, uint32_t* out) {
  Device& d = g_devs[di];
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(d, lk);
  LaneDrain drain(l);
  int rc;
  if ((rc = lane_stream(l))) return rc;
  const uint32_t* gtab = nullptr;
  if ((rc = ec_gtab(d, l, &gtab))) return rc;
  // consecutive launches of at most per_launch blocks keep the tables under the cap; one block always runs
  const size_t block_bytes = (size_t)n_points * kEcMsmPointBytes;
  const uint32_t blocks = (count + 63u) / 64u;
  const uint32_t per_launch =
      (uint32_t)std::min<size_t>(blocks, std::max<size_t>(1, ((size_t)g_ec_msm_ws_mb << 20) / block_bytes));
  const size_t ab = a ? (size_t)count * 8u * 4u : 0, sb = (size_t)count * n_points * 8u * 4u,
               pb = (size_t)count * n_points * 16u * 4u, ob = (size_t)count * 16u * 4u;
  if ((rc = ensure_buffer(l.stage[0], sb)) || (rc = ensure_buffer(l.stage[1], pb)) ||
      (rc = ensure_buffer(l.stage[2], ob)) || (a && (rc = ensure_buffer(l.stage[3], ab))) ||
      (rc = ensure_workspace(l, (size_t)per_launch * block_bytes)))
    return rc;
  if ((rc = h2d(l, l.stage[0].ptr, scalars, sb)) || (rc = h2d(l, l.stage[1].ptr, points, pb)) ||
      (a && (rc = h2d(l, l.stage[3].ptr, a, ab))))
    return rc;
  const uint32_t *d_sc = (const uint32_t*)l.stage[0].ptr, *d_pt = (const uint32_t*)l.stage[1].ptr,
                 *d_a = a ? (const uint32_t*)l.stage[3].ptr : nullptr;
  uint32_t* d_out = (uint32_t*)l.stage[2].ptr;
  for (uint32_t b0 = 0; b0 < blocks; b0 += per_launch) {
    const uint32_t first = b0 * 64u, n = std::min(count - first, per_launch * 64u);
    const int ks = kstat_begin(l);
    hipError_t e = mpcx_launch_ec_msm(d_a ? d_a + (size_t)first * 8u : nullptr, d_sc + (size_t)first * n_points * 8u,
                                      d_pt + (size_t)first * n_points * 16u, d_out + (size_t)first * 16u, gtab, l.ws,
                                      n, n_points, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_ec_msm");
    kstat_end(l, ks, d, di, "ec_msm", -1, n, 0.0);
    d.launches.fetch_add(1, std::memory_order_relaxed);
    launch_log("ec_msm", -1, n, 256, 256, 0.0);
  }
  return d2h_sync(out, l.stage[2].ptr, ob, l);
}
}  // namespace

int mpcx_ec_msm_batch(uint32_t count, uint32_t n_points, const uint32_t* a, const uint32_t* scalars,
                      const uint32_t* points, uint32_t* out) {
  if (n_points < 1 || n_points > MPCX_EC_MSM_MAX_POINTS)
    return fail(MPCX_EINVAL, "n_points %u outside [1, %d]", n_points, MPCX_EC_MSM_MAX_POINTS);
  if (!scalars || !points || !out) return fail(MPCX_EINVAL, "null buffer");
  if (count == 0) return MPCX_OK;
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t n) {
    return ec_msm_range(di, n, n_points, a ? a + (size_t)first * 8u : nullptr,
                        scalars + (size_t)first * n_points * 8u, points + (size_t)first * n_points * 16u,
                        out + (size_t)first * 16u);
  });
}

// One field or point operation of mpcx_ec_fe.hpp per item (k_ec_probe), on the
// thread's selected device; for tests and tools.
int mpcx_ec_probe(uint32_t op, uint32_t count, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (op > MPCX_EC_OP_JAC_MADD) return fail(MPCX_EINVAL, "unknown secp256k1 probe op %u", op);
  if (!a || !b || !out) return fail(MPCX_EINVAL, "null buffer");
  if (count == 0) return MPCX_OK;
  // every input value < p = 2^256 - 2^32 - 977: limbs 2..7 all ones and (limb 1, limb 0) >= (p1, p0) is >= p
  for (int s = 0; s < 2; ++s) {
    const uint32_t* in = s ? b : a;
    for (size_t e = 0; e < (size_t)count * 3u; ++e) {
      const uint32_t* v = in + e * 8u;
      uint32_t hi = 0xFFFFFFFFu;
      for (int i = 2; i < 8; ++i) hi &= v[i];
      if (hi == 0xFFFFFFFFu && (v[1] == 0xFFFFFFFFu || (v[1] == 0xFFFFFFFEu && v[0] >= 0xFFFFFC2Fu)))
        return fail(MPCX_EINVAL, "item %zu: value %zu of input %c is >= p", e / 3u, e % 3u, s ? 'b' : 'a');
    }
  }
  Device* dev = nullptr;
  int rc;
  if ((rc = selected(&dev))) return rc;
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(*dev, lk);
  LaneDrain drain(l);
  if ((rc = lane_stream(l))) return rc;
  const size_t nb = (size_t)count * 24u * 4u;
  if ((rc = ensure_buffer(l.stage[0], nb)) || (rc = ensure_buffer(l.stage[1], nb)) ||
      (rc = ensure_buffer(l.stage[2], nb)))
    return rc;
  if ((rc = h2d(l, l.stage[0].ptr, a, nb)) || (rc = h2d(l, l.stage[1].ptr, b, nb))) return rc;
  const hipError_t e = mpcx_launch_ec_probe(op, (const uint32_t*)l.stage[0].ptr, (const uint32_t*)l.stage[1].ptr,
                                            (uint32_t*)l.stage[2].ptr, count, l.st);
  if (e != hipSuccess) return hip_fail(e, "launch k_ec_probe");
  return d2h_sync(out, l.stage[2].ptr, nb, l);
}

// ------------------------------------------------------------ Ed25519
namespace {
// the base point B of RFC 8032 (x, y)
constexpr uint32_t kEdB[16] = {0x8F25D51Au, 0xC9562D60u, 0x9525A7B2u, 0x692CC760u, 0xFDD6DC5Cu, 0xC0A4E231u,
                               0xCD6E53FEu, 0x216936D3u, 0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                               0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
// k_ed_msm's per-thread tables: 15 entries of 32 words (Y + X, Y - X, 2 Z, 2 d T) per point, 64 lanes per block
constexpr size_t kEdMsmPointBytes = 15u * 32u * 64u * 4u;

// The Ed25519 base-point comb of device d, built on first use as ec_gtab is:
// entry (w, v) = (v 2^(8w)) B as a plain scalar multiple of B by k_ed_msm
// itself, then every affine result turned into its mixed-addition entry. The
// caller holds lane l.
int ed_btab(Device& d, Lane& l, const uint32_t** out) {
  std::lock_guard<std::mutex> lk(d.ec_mu);
  if (!d.ed_btab) {
    std::vector<uint32_t> sc((size_t)kEcTabEntries * 8u, 0u), pts((size_t)kEcTabEntries * 16u, 0u);
    for (uint32_t w = 0; w < 32; ++w)
      for (uint32_t v = 1; v <= 255; ++v) {
        const size_t e = (size_t)w * 255u + (v - 1u);
        sc[e * 8u + w / 4u] = v << (8u * (w % 4u));
        std::memcpy(&pts[e * 16u], kEdB, sizeof kEdB);
      }
    int rc;
    const size_t sb = sc.size() * 4, pb = pts.size() * 4, ob = (size_t)kEcTabEntries * 16u * 4u;
    if ((rc = ensure_buffer(l.stage[0], sb)) || (rc = ensure_buffer(l.stage[1], pb)) ||
        (rc = ensure_buffer(l.stage[2], ob)) ||
        (rc = ensure_workspace(l, (size_t)((kEcTabEntries + 63u) / 64u) * kEdMsmPointBytes)))
      return rc;
    uint32_t* tab = nullptr;
    hipError_t e = hipMalloc((void**)&tab, (size_t)kEcTabEntries * 24u * 4u);
    if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(Ed25519 comb): %s", hipGetErrorString(e));
    if ((rc = h2d(l, l.stage[0].ptr, sc.data(), sb)) || (rc = h2d(l, l.stage[1].ptr, pts.data(), pb))) {
      (void)hipFree(tab);
      return rc;
    }
    e = mpcx_launch_ed_msm(nullptr, (const uint32_t*)l.stage[0].ptr, (const uint32_t*)l.stage[1].ptr,
                           (uint32_t*)l.stage[2].ptr, nullptr, l.ws, kEcTabEntries, 1u, l.st);
    if (e == hipSuccess)
      e = mpcx_launch_ed_comb_entries((const uint32_t*)l.stage[2].ptr, tab, kEcTabEntries, l.st);
    if (e != hipSuccess) {
      (void)hipFree(tab);
      return hip_fail(e, "launch k_ed_msm (comb build)");
    }
    if ((rc = lane_wait(l))) {
      (void)hipFree(tab);
      return rc;
    }
    d.ed_btab = tab;
  }
  *out = d.ed_btab;
  return MPCX_OK;
}

int ed_msm_range(int di, uint32_t count, uint32_t n_points, const uint32_t* a, const uint32_t* scalars,
                 const uint32_t* points, uint32_t* out) {
  Device& d = g_devs[di];
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(d, lk);
  LaneDrain drain(l);
  int rc;
  if ((rc = lane_stream(l))) return rc;
  const uint32_t* btab = nullptr;
  if ((rc = ed_btab(d, l, &btab))) return rc;
  // consecutive launches of at most per_launch blocks keep the tables under the cap; one block always runs
  const size_t block_bytes = (size_t)n_points * kEdMsmPointBytes;
  const uint32_t blocks = (count + 63u) / 64u;
  const uint32_t per_launch =
      block_bytes ? (uint32_t)std::min<size_t>(blocks, std::max<size_t>(1, ((size_t)g_ec_msm_ws_mb << 20) / block_bytes))
                  : blocks;
  const size_t ab = a ? (size_t)count * 8u * 4u : 0, sb = (size_t)count * n_points * 8u * 4u,
               pb = (size_t)count * n_points * 16u * 4u, ob = (size_t)count * 16u * 4u;
  if ((n_points && ((rc = ensure_buffer(l.stage[0], sb)) || (rc = ensure_buffer(l.stage[1], pb)) ||
                    (rc = ensure_workspace(l, (size_t)per_launch * block_bytes)))) ||
      (rc = ensure_buffer(l.stage[2], ob)) || (a && (rc = ensure_buffer(l.stage[3], ab))))
    return rc;
  if ((n_points && ((rc = h2d(l, l.stage[0].ptr, scalars, sb)) || (rc = h2d(l, l.stage[1].ptr, points, pb)))) ||
      (a && (rc = h2d(l, l.stage[3].ptr, a, ab))))
    return rc;
  const uint32_t *d_sc = n_points ? (const uint32_t*)l.stage[0].ptr : nullptr,
                 *d_pt = n_points ? (const uint32_t*)l.stage[1].ptr : nullptr,
                 *d_a = a ? (const uint32_t*)l.stage[3].ptr : nullptr;
  uint32_t* d_out = (uint32_t*)l.stage[2].ptr;
  for (uint32_t b0 = 0; b0 < blocks; b0 += per_launch) {
    const uint32_t first = b0 * 64u, n = std::min(count - first, per_launch * 64u);
    const int ks = kstat_begin(l);
    hipError_t e = mpcx_launch_ed_msm(d_a ? d_a + (size_t)first * 8u : nullptr,
                                      d_sc ? d_sc + (size_t)first * n_points * 8u : nullptr,
                                      d_pt ? d_pt + (size_t)first * n_points * 16u : nullptr,
                                      d_out + (size_t)first * 16u, btab, n_points ? l.ws : nullptr, n, n_points, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_ed_msm");
    kstat_end(l, ks, d, di, "ed_msm", -1, n, 0.0);
    d.launches.fetch_add(1, std::memory_order_relaxed);
    launch_log("ed_msm", -1, n, 256, 256, 0.0);
  }
  return d2h_sync(out, l.stage[2].ptr, ob, l);
}

// v (8 words) >= p = 2^255 - 19
bool ed_geq_p(const uint32_t* v) {
  if (v[7] >> 31) return true;
  uint32_t hi = v[7] | 0x80000000u;
  for (int i = 1; i < 7; ++i) hi &= v[i];
  return hi == 0xFFFFFFFFu && v[0] >= 0xFFFFFFEDu;
}
}  // namespace

int mpcx_ed_msm_batch(uint32_t count, uint32_t n_points, const uint32_t* a, const uint32_t* scalars,
                      const uint32_t* points, uint32_t* out) {
  if (n_points > MPCX_ED_MSM_MAX_POINTS)
    return fail(MPCX_EINVAL, "n_points %u outside [0, %d]", n_points, MPCX_ED_MSM_MAX_POINTS);
  if (n_points == 0 && !a) return fail(MPCX_EINVAL, "n_points 0 needs the base-point scalars a");
  if (!out || (n_points && (!scalars || !points))) return fail(MPCX_EINVAL, "null buffer");
  if (count == 0) return MPCX_OK;
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t n) {
    return ed_msm_range(di, n, n_points, a ? a + (size_t)first * 8u : nullptr,
                        n_points ? scalars + (size_t)first * n_points * 8u : nullptr,
                        n_points ? points + (size_t)first * n_points * 16u : nullptr, out + (size_t)first * 16u);
  });
}

namespace {
int ed_admit_range(int di, uint32_t count, uint32_t clear, const uint32_t* points, uint32_t* out, uint8_t* status) {
  Device& d = g_devs[di];
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(d, lk);
  LaneDrain drain(l);
  int rc;
  if ((rc = lane_stream(l))) return rc;
  const size_t pb = (size_t)count * 16u * 4u;
  if ((rc = ensure_buffer(l.stage[0], pb)) || (rc = ensure_buffer(l.stage[2], pb)) ||
      (rc = ensure_buffer(l.stage[3], count)))
    return rc;
  if ((rc = h2d(l, l.stage[0].ptr, points, pb))) return rc;
  const int ks = kstat_begin(l);
  const hipError_t e = mpcx_launch_ed_admit((const uint32_t*)l.stage[0].ptr, (uint32_t*)l.stage[2].ptr,
                                            (uint8_t*)l.stage[3].ptr, count, clear, l.st);
  if (e != hipSuccess) return hip_fail(e, "launch k_ed_admit");
  kstat_end(l, ks, d, di, "ed_admit", -1, count, 0.0);
  d.launches.fetch_add(1, std::memory_order_relaxed);
  launch_log("ed_admit", -1, count, 256, 256, 0.0);
  if ((rc = d2h(l, status, l.stage[3].ptr, count))) return rc;
  return d2h_sync(out, l.stage[2].ptr, pb, l);
}
}  // namespace

int mpcx_ed_admit_batch(uint32_t count, uint32_t clear, const uint32_t* points, uint32_t* out, uint8_t* status) {
  if (clear > 1) return fail(MPCX_EINVAL, "clear %u is not 0 or 1", clear);
  if (!points || !out || !status) return fail(MPCX_EINVAL, "null buffer");
  if (count == 0) return MPCX_OK;
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t n) {
    return ed_admit_range(di, n, clear, points + (size_t)first * 16u, out + (size_t)first * 16u, status + first);
  });
}

// One field or point operation of mpcx_ed_fe.hpp per item (k_ed_probe), on the
// thread's selected device; for tests and tools.
int mpcx_ed_probe(uint32_t op, uint32_t count, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (op > MPCX_ED_OP_ED_MADD) return fail(MPCX_EINVAL, "unknown Ed25519 probe op %u", op);
  if (!a || !b || !out) return fail(MPCX_EINVAL, "null buffer");
  if (count == 0) return MPCX_OK;
  for (int s = 0; s < 2; ++s) {
    const uint32_t* in = s ? b : a;
    for (size_t e = 0; e < (size_t)count * 4u; ++e)
      if (ed_geq_p(in + e * 8u))
        return fail(MPCX_EINVAL, "item %zu: value %zu of input %c is >= p", e / 4u, e % 4u, s ? 'b' : 'a');
  }
  Device* dev = nullptr;
  int rc;
  if ((rc = selected(&dev))) return rc;
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(*dev, lk);
  LaneDrain drain(l);
  if ((rc = lane_stream(l))) return rc;
  const size_t nb = (size_t)count * 32u * 4u;
  if ((rc = ensure_buffer(l.stage[0], nb)) || (rc = ensure_buffer(l.stage[1], nb)) ||
      (rc = ensure_buffer(l.stage[2], nb)))
    return rc;
  if ((rc = h2d(l, l.stage[0].ptr, a, nb)) || (rc = h2d(l, l.stage[1].ptr, b, nb))) return rc;
  const hipError_t e = mpcx_launch_ed_probe(op, (const uint32_t*)l.stage[0].ptr, (const uint32_t*)l.stage[1].ptr,
                                            (uint32_t*)l.stage[2].ptr, count, l.st);
  if (e != hipSuccess) return hip_fail(e, "launch k_ed_probe");
  return d2h_sync(out, l.stage[2].ptr, nb, l);
}

int mpcx_fermat2_batch(uint32_t count, const uint32_t* p, uint32_t p_words, uint8_t* ok) {
  if (count == 0) return MPCX_OK;
  if (!p || !ok || p_words == 0) return fail(MPCX_EINVAL, "null buffer");
  if (p_words > (uint32_t)MPCX_CLASS_WORDS(0))
    return fail(MPCX_EINVAL, "p_words %u > %d", p_words, MPCX_CLASS_WORDS(0));
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t* pi = p + (size_t)i * p_words;
    const uint32_t bits = bit_length_words(pi, p_words);
    if (bits > (uint32_t)MPCX_CLASS_MAXBITS(0))
      return fail(MPCX_EINVAL, "candidate %u has %u bits > %d", i, bits, MPCX_CLASS_MAXBITS(0));
    if (bits < 3 || (pi[0] & 1u) == 0) return fail(MPCX_EINVAL, "candidate %u is not an odd integer >= 5", i);
  }
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t n) {
    std::unique_lock<std::mutex> lk;
    Lane& l = acquire_lane(g_devs[di], lk);
    LaneDrain drain(l);
    int rc;
    if ((rc = lane_stream(l))) return rc;
    const size_t pb = (size_t)n * p_words * 4;
    if ((rc = ensure_buffer(l.stage[0], pb)) || (rc = ensure_buffer(l.stage[3], n)) ||
        (rc = ensure_buffer(l.stage[1], (size_t)n * MPCX_PRIME_L * 4)) ||
        (rc = ensure_buffer(l.stage[2], (size_t)n * 8)))
      return rc;
    if ((rc = h2d(l, l.stage[0].ptr, p + (size_t)first * p_words, pb))) return rc;
    mpcx::Prime2Args a{};
    a.nf = (const uint32_t*)l.stage[0].ptr;
    a.count_f = n;
    a.ok_f = (uint8_t*)l.stage[3].ptr;
    a.n_words = p_words;
    a.r1 = (uint32_t*)l.stage[1].ptr;
    a.meta = (uint32_t*)l.stage[2].ptr;
    const hipError_t e = mpcx_launch_prime2c(a, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_prime2c");
    return d2h_sync(ok + first, l.stage[3].ptr, n, l);
  });
}

int mpcx_mr_batch(uint32_t count, const uint32_t* n, uint32_t n_words, const uint32_t* bases, uint8_t* ok) {
  if (count == 0) return MPCX_OK;
  if (!n || !bases || !ok || n_words == 0) return fail(MPCX_EINVAL, "null buffer");
  if (n_words > (uint32_t)MPCX_CLASS_WORDS(0))
    return fail(MPCX_EINVAL, "n_words %u > %d", n_words, MPCX_CLASS_WORDS(0));
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t* ni = n + (size_t)i * n_words;
    if (bit_length_words(ni, n_words) < 3 || (ni[0] & 1u) == 0)
      return fail(MPCX_EINVAL, "candidate %u is not an odd integer >= 5", i);
  }
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t cnt) {
    std::unique_lock<std::mutex> lk;
    Lane& l = acquire_lane(g_devs[di], lk);
    LaneDrain drain(l);
    int rc;
    if ((rc = lane_stream(l))) return rc;
    const size_t nb = (size_t)cnt * n_words * 4;
    if ((rc = ensure_buffer(l.stage[0], nb)) || (rc = ensure_buffer(l.stage[1], nb)) ||
        (rc = ensure_buffer(l.stage[3], cnt)) || (rc = ensure_buffer(l.stage[2], (size_t)cnt * (MPCX_MR_L + 2) * 4)))
      return rc;
    if ((rc = h2d(l, l.stage[0].ptr, n + (size_t)first * n_words, nb)) ||
        (rc = h2d(l, l.stage[1].ptr, bases + (size_t)first * n_words, nb)))
      return rc;
    mpcx::MrArgs a{};
    a.n = (const uint32_t*)l.stage[0].ptr;
    a.a = (const uint32_t*)l.stage[1].ptr;
    a.ok = (uint8_t*)l.stage[3].ptr;
    a.count = cnt;
    a.n_words = n_words;
    a.r1 = (uint32_t*)l.stage[2].ptr;
    a.meta = a.r1 + (size_t)cnt * MPCX_MR_L;
    const hipError_t e = mpcx_launch_mrc(&a, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_mrc");
    return d2h_sync(ok + first, l.stage[3].ptr, cnt, l);
  });
}

int mpcx_lucas_batch(uint32_t count, const uint32_t* n, uint32_t n_words, const uint32_t* P, uint8_t* ok) {
  if (count == 0) return MPCX_OK;
  if (!n || !P || !ok || n_words == 0) return fail(MPCX_EINVAL, "null buffer");
  if (n_words > 64u) return fail(MPCX_EINVAL, "n_words %u > 64", n_words);
  uint32_t maxbits = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t* ni = n + (size_t)i * n_words;
    const uint32_t bits = bit_length_words(ni, n_words);
    if (bits < 3 || (ni[0] & 1u) == 0) return fail(MPCX_EINVAL, "candidate %u is not an odd integer >= 5", i);
    if (bits > 2048) return fail(MPCX_EINVAL, "candidate %u has %u bits > 2048", i, bits);
    if (P[i] < 3 || P[i] >= (1u << 14)) return fail(MPCX_EINVAL, "Lucas parameter P[%u] = %u outside [3, 2^14)", i, P[i]);
    maxbits = std::max(maxbits, bits);
  }
  // candidates above 1024 bits: the wide geometry (16 x 5 digits)
  const bool wide = maxbits > 1024;
  const uint32_t cl = wide ? (uint32_t)MPCX_LUCASW_L : (uint32_t)MPCX_MR_L;
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t cnt) {
    std::unique_lock<std::mutex> lk;
    Lane& l = acquire_lane(g_devs[di], lk);
    LaneDrain drain(l);
    int rc;
    if ((rc = lane_stream(l))) return rc;
    const size_t nb = (size_t)cnt * n_words * 4;
    if ((rc = ensure_buffer(l.stage[0], nb)) || (rc = ensure_buffer(l.stage[1], (size_t)cnt * 4)) ||
        (rc = ensure_buffer(l.stage[3], cnt)) || (rc = ensure_buffer(l.stage[2], (size_t)cnt * (4 * cl + 2) * 4)))
      return rc;
    if ((rc = h2d(l, l.stage[0].ptr, n + (size_t)first * n_words, nb)) ||
        (rc = h2d(l, l.stage[1].ptr, P + first, (size_t)cnt * 4)))
      return rc;
    mpcx::LucasArgs a{};
    a.n = (const uint32_t*)l.stage[0].ptr;
    a.P = (const uint32_t*)l.stage[1].ptr;
    a.ok = (uint8_t*)l.stage[3].ptr;
    a.count = cnt;
    a.n_words = n_words;
    a.consts = (uint32_t*)l.stage[2].ptr;
    a.meta = a.consts + (size_t)cnt * 4 * cl;
    const hipError_t e = wide ? mpcx_launch_lucasc_wide(&a, l.st) : mpcx_launch_lucasc(&a, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_lucasc");
    return d2h_sync(ok + first, l.stage[3].ptr, cnt, l);
  });
}

int mpcx_dev_alloc(size_t bytes, void** out_ptr) {
  if (!out_ptr) return fail(MPCX_EINVAL, "null out_ptr");
  Device* dev = nullptr;
  if (int rc = selected(&dev)) return rc;
  hipError_t e = hipMalloc(out_ptr, bytes);
  if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  return MPCX_OK;
}

int mpcx_dev_free(void* ptr) {
  hipError_t e = hipFree(ptr);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "hipFree");
}

int mpcx_host_alloc(size_t bytes, void** out_ptr) {
  if (!out_ptr) return fail(MPCX_EINVAL, "null out_ptr");
  Device* dev = nullptr;
  if (int rc = selected(&dev)) return rc;
  hipError_t e = hipHostMalloc(out_ptr, std::max<size_t>(bytes, 1), hipHostMallocPortable);
  if (e != hipSuccess) return fail(MPCX_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
  g_pins.add(*out_ptr, std::max<size_t>(bytes, 1));
  return MPCX_OK;
}

int mpcx_host_free(void* ptr) {
  if (!ptr) return MPCX_OK;
  g_pins.remove(ptr);
  hipError_t e = hipHostFree(ptr);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "hipHostFree");
}

int mpcx_copy_stats(uint64_t* direct_bytes, uint64_t* bounced_bytes, uint64_t* bounce_allocs) {
  if (direct_bytes) *direct_bytes = g_cp_direct.load(std::memory_order_relaxed);
  if (bounced_bytes) *bounced_bytes = g_cp_bounced.load(std::memory_order_relaxed);
  if (bounce_allocs) *bounce_allocs = g_cp_bounce_grow.load(std::memory_order_relaxed);
  return MPCX_OK;
}

int mpcx_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
  // the null stream: ordered after earlier blocking-stream work (hipMemcpy's semantics)
  return copy_sync(d_dst, h_src, bytes, hipMemcpyHostToDevice, nullptr);
}

int mpcx_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
  return copy_sync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, nullptr);
}

int mpcx_stream_create(void** out_stream) {
  if (!out_stream) return fail(MPCX_EINVAL, "null out_stream");
  Device* dev = nullptr;
  if (int rc = selected(&dev)) return rc;
  hipStream_t s;
  hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
  *out_stream = (void*)s;
  return MPCX_OK;
}

int mpcx_stream_destroy(void* stream) {
  // drop the device-buffer workspace this stream owned on every device
  const int n = g_ndev.load();
  for (int i = 0; i < n; ++i) {
    Device& d = g_devs[i];
    std::unique_ptr<Lane> l;
    {
      std::lock_guard<std::mutex> lk(d.dev_mu);
      auto it = d.dev_lanes.find((hipStream_t)stream);
      if (it == d.dev_lanes.end()) continue;
      l = std::move(it->second);
      d.dev_lanes.erase(it);
    }
    if (bind(d) == MPCX_OK) drop_lane(*l);
  }
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "hipStreamDestroy");
}

int mpcx_stream_sync(void* stream) {
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  return e == hipSuccess ? MPCX_OK : hip_fail(e, "hipStreamSynchronize");
}

int mpcx_sync(void* stream) { return mpcx_stream_sync(stream); }

}  // extern "C"

// ------------------------------------------------------------ fixed base
// Comb tables for a long-lived base (h1, h2 of a node's N~; SURVEY.md 8(a)
// "shared bases"): entry (j, v) = b^(v 2^(8j)) R mod m. Built on the GPU by
// the modexp kernels on the selected device: b_j = b^(2^(8j)) (per-operand
// exponents), then T(j, v) = (R mod m) * b_j^v (fused multiplier), then
// reordered into the kernel geometry's digit layout on the host; the host copy
// is kept so other bound devices receive the table on first use.
constexpr size_t kFbBuildSlice = 65536;  // table entries per build launch

int mpcx_fixedbase_register(mpcx_mod_t mod, const uint32_t* base, uint32_t base_words, uint32_t max_exp_bits,
                            mpcx_fb_t* out) {
  if (!mod || !base || !out) return fail(MPCX_EINVAL, "null argument");
  if (mod->cls > 1) return fail(MPCX_EINVAL, "fixed-base tables serve moduli of <= %d bits", MPCX_CLASS_MAXBITS(1));
  const uint32_t cw = (uint32_t)MPCX_CLASS_WORDS(mod->cls);
  if (base_words == 0 || base_words > cw) return fail(MPCX_EINVAL, "base_words %u outside [1, %u]", base_words, cw);
  if (max_exp_bits == 0 || max_exp_bits > MPCX_FB_MAX_EXP_BITS)
    return fail(MPCX_EINVAL, "max_exp_bits %u outside [1, %d]", max_exp_bits, MPCX_FB_MAX_EXP_BITS);
  Device* dev = nullptr;
  if (int rc = selected(&dev)) return rc;
  const int di = (int)(dev - g_devs);
  Lane& bl = dev->build_lane;
  std::lock_guard<std::mutex> blk(bl.mu);
  LaneDrain drain(bl);
  int rc;
  if ((rc = lane_stream(bl))) return rc;
  const int geom = fb_geom_for(mod);  // the comb tables' layout
  const uint32_t L = (uint32_t)MPCX_GEOM_L(geom), P = (uint32_t)MPCX_GEOM_P(geom), K = (uint32_t)MPCX_GEOM_K(geom);
  // window width: the configured one, narrowed until the table fits
  // MPCX_FB_MAX_TABLE_BYTES (one product per window; 2^w entries per window)
  uint32_t wb = (uint32_t)g_fb_window;
  auto tbytes = [&](uint32_t w) {
    return (unsigned long long)((max_exp_bits + w - 1) / w) * (1ull << w) * L * 4ull;
  };
  while (wb > 4 && tbytes(wb) > MPCX_FB_MAX_TABLE_BYTES) --wb;
  const uint32_t nwin = (max_exp_bits + wb - 1) / wb;
  const uint32_t entries = 1u << wb;
  const uint32_t nv = entries - 1;  // v = 1..2^w-1 computed; v = 0 is R mod m
  const size_t n2 = (size_t)nwin * nv;
  if (n2 > 0xFFFFFFFFull) return fail(MPCX_EINVAL, "table too large");
  const uint32_t ew1 = (wb * (nwin - 1)) / 32 + 1;  // 2^(w j) needs bit w j
  // host inputs
  std::vector<uint32_t> hb((size_t)nwin * cw, 0), he1((size_t)nwin * ew1, 0);
  for (uint32_t j = 0; j < nwin; ++j) {
    std::memcpy(&hb[(size_t)j * cw], base, base_words * 4);
    const uint32_t bit = wb * j;
    he1[(size_t)j * ew1 + bit / 32] = 1u << (bit % 32);
  }
  const std::vector<uint32_t> r1w = pow2_mod(kDigitBits * L, mod->m);  // R mod m, mod->words words
  std::vector<uint32_t> he2(n2), hm(n2 * mod->words);
  for (size_t i = 0; i < n2; ++i) {
    he2[i] = (uint32_t)(i % nv) + 1u;
    std::memcpy(&hm[i * mod->words], r1w.data(), mod->words * 4);
  }
  uint32_t *d_b = nullptr, *d_e1 = nullptr, *d_bj = nullptr, *d_e2 = nullptr, *d_m = nullptr, *d_t = nullptr;
  auto cleanup = [&] {
    for (uint32_t* ptr : {d_b, d_e1, d_bj, d_e2, d_m, d_t})
      if (ptr) (void)hipFree(ptr);
  };
  auto alloc = [&](uint32_t** ptr, size_t words) {
    return hipMalloc((void**)ptr, std::max<size_t>(words, 1) * 4) == hipSuccess;
  };
  if (!alloc(&d_b, hb.size()) || !alloc(&d_e1, he1.size()) || !alloc(&d_bj, (size_t)nwin * cw) ||
      !alloc(&d_e2, n2) || !alloc(&d_m, hm.size()) || !alloc(&d_t, n2 * cw)) {
    cleanup();
    return fail(MPCX_ENOMEM, "hipMalloc(fixed-base build)");
  }
  if ((rc = copy_sync(d_b, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, bl.st)) ||
      (rc = copy_sync(d_e1, he1.data(), he1.size() * 4, hipMemcpyHostToDevice, bl.st)) ||
      (rc = copy_sync(d_e2, he2.data(), he2.size() * 4, hipMemcpyHostToDevice, bl.st)) ||
      (rc = copy_sync(d_m, hm.data(), hm.size() * 4, hipMemcpyHostToDevice, bl.st))) {
    cleanup();
    return rc;
  }
  rc = modexp_enqueue(di, bl, mod, nwin, d_b, cw, d_e1, ew1, 0, wb * (nwin - 1) + 1, nullptr, 0, d_bj, cw, false);
  // T(j, v) = R * b_j^v: operand i = j*nv + (v-1) takes base b_j -> replicate b_j rows
  std::vector<uint32_t> hbj((size_t)nwin * cw), hb2;
  if (!rc) rc = lane_wait(bl);
  if (!rc) rc = copy_sync(hbj.data(), d_bj, hbj.size() * 4, hipMemcpyDeviceToHost, bl.st);
  if (!rc) {
    hb2.resize(n2 * cw);
    for (size_t i = 0; i < n2; ++i) std::memcpy(&hb2[i * cw], &hbj[(i / nv) * cw], cw * 4);
    (void)hipFree(d_b);
    d_b = nullptr;
    if (!alloc(&d_b, hb2.size())) rc = fail(MPCX_ENOMEM, "hipMalloc(fixed-base bases)");
  }
  if (!rc) rc = copy_sync(d_b, hb2.data(), hb2.size() * 4, hipMemcpyHostToDevice, bl.st);
  if (!rc)
    // in slices: the build lane's window-table workspace grows with the
    // operands of one launch (a 12-bit table has ~1M entries)
    for (size_t off = 0; off < n2 && !rc; off += kFbBuildSlice) {
      const uint32_t cnt = (uint32_t)std::min<size_t>(kFbBuildSlice, n2 - off);
      rc = modexp_enqueue(di, bl, mod, cnt, d_b + off * cw, cw, d_e2 + off, 1, 0, wb, d_m + off * mod->words,
                          mod->words, d_t + off * cw, cw, false);
    }
  std::vector<uint32_t> ht(n2 * cw);
  if (!rc) rc = lane_wait(bl);
  if (!rc) rc = copy_sync(ht.data(), d_t, ht.size() * 4, hipMemcpyDeviceToHost, bl.st);
  cleanup();
  if (rc) return rc;
  auto* fb = new mpcx_fixedbase_s();
  fb->mod = mod;
  fb->geom = geom;
  fb->nwin = nwin;
  fb->wbits = wb;
  // digits, [k][p] interleaved per entry (a group's P lanes read P consecutive words per slot)
  const size_t ent_words = L;
  auto& tab = fb->host_table;
  fb->table_words = (size_t)nwin * entries * ent_words;
  tab.assign(fb->table_words, 0);
  auto put = [&](size_t ent, const std::vector<uint32_t>& words) {
    const std::vector<uint32_t> d = to_digits(words, L);
    uint32_t* dst = &tab[ent * ent_words];
    for (uint32_t pp = 0; pp < P; ++pp)
      for (uint32_t k = 0; k < K; ++k) dst[k * P + pp] = d[pp * K + k];
  };
  // 2^w entries per window: the conversion to interleaved digits runs on the
  // host threads (a 12-bit table is ~1M entries)
  const uint32_t nthr = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> conv;
  for (uint32_t t = 0; t < nthr; ++t)
    conv.emplace_back([&, t] {
      std::vector<uint32_t> w(cw);
      for (uint32_t j = t; j < nwin; j += nthr) {
        put((size_t)j * entries, r1w);
        for (uint32_t v = 1; v < entries; ++v) {
          std::memcpy(w.data(), &ht[((size_t)j * nv + (v - 1)) * cw], cw * 4);
          put((size_t)j * entries + v, w);
        }
      }
    });
  for (auto& th : conv) th.join();
  const uint32_t* dt = nullptr;
  if ((rc = fb_table(fb, di, &dt))) {
    delete fb;
    return rc;
  }
  *out = fb;
  return MPCX_OK;
}

int mpcx_fixedbase_release(mpcx_fb_t fb) {
  if (!fb) return fail(MPCX_EINVAL, "null fixed base");
  const int n = g_ndev.load();
  for (int i = 0; i < n && i < kMaxDevices; ++i)
    if (fb->d_table[i] && bind(g_devs[i]) == MPCX_OK) (void)hipFree(fb->d_table[i]);
  delete fb;
  return MPCX_OK;
}

int mpcx_fixedbase_info(mpcx_fb_t fb, uint32_t* max_exp_bits, size_t* table_bytes) {
  if (!fb) return fail(MPCX_EINVAL, "null fixed base");
  if (max_exp_bits) *max_exp_bits = fb->nwin * fb->wbits;
  if (table_bytes) *table_bytes = ((size_t)fb->nwin << fb->wbits) * MPCX_GEOM_L(fb->geom) * 4;
  return MPCX_OK;
}

int mpcx_fixedbase_exp_batch(uint32_t nbases, const mpcx_fb_t* fbs, uint32_t count, const uint32_t* const* exps,
                             const uint32_t* exp_words, const uint32_t* muls, uint32_t mul_words, uint32_t* out,
                             uint32_t out_words) {
  mpcx_fixedbase_group_t g{};  // the call as one group
  g.nbases = nbases;
  if (nbases >= 1 && nbases <= MPCX_FB_MAX_BASES) {  // otherwise fb_group_check fails before it reads the arrays
    if (!fbs || !exps || !exp_words) return fail(MPCX_EINVAL, "null argument");
    for (uint32_t t = 0; t < nbases; ++t) {
      g.fbs[t] = fbs[t];
      g.exps[t] = exps[t];
      g.exp_words[t] = exp_words[t];
    }
  }
  g.count = count;
  g.muls = muls;
  g.mul_words = mul_words;
  g.out = out;
  g.out_words = out_words;
  uint32_t nwin[MPCX_FB_MAX_BASES] = {0, 0};
  if (int rc = fb_group_check(g, "", nwin)) return rc;
  if (count == 0) return MPCX_OK;
  return run_sliced(count, g_split_min, [&](int di, uint32_t first, uint32_t n) {
    mpcx_fixedbase_group_t s = g;  // this device's slice
    s.count = n;
    for (uint32_t t = 0; t < nbases; ++t) s.exps[t] = g.exps[t] + (size_t)first * g.exp_words[t];
    if (muls) s.muls = muls + (size_t)first * mul_words;
    s.out = out + (size_t)first * out_words;
    const size_t eb[MPCX_FB_MAX_BASES] = {(size_t)n * s.exp_words[0] * 4, (size_t)n * s.exp_words[1] * 4};
    const size_t ob = (size_t)n * out_words * 4, mb = muls ? (size_t)n * mul_words * 4 : 0;
    std::unique_lock<std::mutex> lk;
    Lane& l = acquire_lane(g_devs[di], lk);
    LaneDrain drain(l);
    int rc;
    if ((rc = lane_stream(l))) return rc;
    Staging* sg = l.stage;
    if ((rc = ensure_buffer(sg[0], eb[0])) || (rc = ensure_buffer(sg[1], eb[1])) ||
        (rc = ensure_buffer(sg[2], ob)) || (muls && (rc = ensure_buffer(sg[3], mb))))
      return rc;
    for (uint32_t t = 0; t < nbases; ++t)
      if (eb[t] && (rc = h2d(l, sg[t].ptr, s.exps[t], eb[t]))) return rc;
    if (muls && (rc = h2d(l, sg[3].ptr, s.muls, mb))) return rc;
    const int geom = s.fbs[0]->geom;
    const uint32_t* d_exps[MPCX_FB_MAX_BASES] = {(const uint32_t*)sg[0].ptr, (const uint32_t*)sg[1].ptr};
    mpcx::FixedBaseArgs a;
    if ((rc = fixedbase_args(s, geom, di, nwin, d_exps, (const uint32_t*)sg[3].ptr, (uint32_t*)sg[2].ptr, &a)))
      return rc;
    const uint32_t blocks = (n + MPCX_GEOM_G(geom) - 1) / MPCX_GEOM_G(geom);
    const uint32_t split = fb_split_for(g_devs[di], blocks);
    const int ks = kstat_begin(l);
    hipError_t e = launch_fixedbase(geom, &a, blocks, split, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_fixedbase");
    g_devs[di].launches.fetch_add(1, std::memory_order_relaxed);
    const FbWork w = fb_group_work(s);
    kstat_end(l, ks, g_devs[di], di, "fixedbase", geom, n, w.exec);
    launch_log("fixedbase", geom, n, s.fbs[0]->mod->bits, w.eb_max, w.alg);
    return d2h_sync(s.out, sg[2].ptr, ob, l);
  });
}

int mpcx_fixedbase_multi_batch(uint32_t n_groups, const mpcx_fixedbase_group_t* gs) {
  if (n_groups == 0) return MPCX_OK;
  if (!gs) return fail(MPCX_EINVAL, "null groups");
  const int n = ndev_or_fail();
  if (n < 0) return -n;
  int cls = -1, rc;
  uint64_t total = 0;
  std::vector<uint32_t> nwin((size_t)n_groups * MPCX_FB_MAX_BASES, 0);
  for (uint32_t i = 0; i < n_groups; ++i) {
    char pre[24];
    std::snprintf(pre, sizeof pre, "group %u: ", i);
    if ((rc = fb_group_check(gs[i], pre, &nwin[(size_t)i * MPCX_FB_MAX_BASES]))) return rc;
    const int c = gs[i].fbs[0]->mod->cls;
    if (cls < 0) cls = c;
    if (c != cls) return fail(MPCX_EINVAL, "group %u: modulus class differs from group 0's", i);
    total += gs[i].count;
  }
  if (total == 0) return MPCX_OK;
  if (total > 0xFFFFFFFFull) return fail(MPCX_EINVAL, "too many operands");
  const int di = (int)(g_dev_rr.fetch_add(1, std::memory_order_relaxed) % (unsigned)n);
  Device& dev = g_devs[di];
  if ((rc = bind(dev))) return rc;
  int geom = -1;  // the tables' layout: one per launch
  for (uint32_t i = 0; i < n_groups; ++i) {
    if (gs[i].count == 0) continue;
    const int g = gs[i].fbs[0]->geom;
    if (geom < 0) geom = g;
    if (g != geom) return fail(MPCX_EINVAL, "group %u: comb table layout differs from group 0's", i);
  }
  const uint32_t G = (uint32_t)MPCX_GEOM_G(geom);
  struct Seg {
    uint32_t gi, waves;
    size_t in_e[MPCX_FB_MAX_BASES], in_m, out_o;
  };
  std::vector<Seg> segs;
  size_t in_words = 0, out_words = 0;
  for (uint32_t i = 0; i < n_groups; ++i) {
    const mpcx_fixedbase_group_t& g = gs[i];
    if (g.count == 0) continue;
    Seg sg{};
    sg.gi = i;
    sg.waves = (g.count + G - 1) / G;
    for (uint32_t t = 0; t < g.nbases; ++t) {
      sg.in_e[t] = in_words;
      in_words += (size_t)g.count * g.exp_words[t];
    }
    sg.in_m = in_words;
    if (g.muls) in_words += (size_t)g.count * g.mul_words;
    sg.out_o = out_words;
    out_words += (size_t)g.count * g.out_words;
    segs.push_back(sg);
  }
  const size_t nseg = segs.size();
  const size_t seg_bytes = nseg * sizeof(mpcx::FixedBaseArgs), first_bytes = (nseg + 1) * sizeof(uint32_t);
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(dev, lk);
  LaneDrain drain(l);
  if ((rc = lane_stream(l))) return rc;
  if ((rc = ensure_buffer(l.stage[0], std::max<size_t>(in_words * 4, 4))) ||
      (rc = ensure_buffer(l.stage[2], out_words * 4)) || (rc = ensure_buffer(l.stage[3], seg_bytes + first_bytes)))
    return rc;
  uint32_t* d_in = (uint32_t*)l.stage[0].ptr;
  uint32_t* d_out = (uint32_t*)l.stage[2].ptr;
  std::vector<mpcx::FixedBaseArgs> args(nseg);
  std::vector<uint32_t> first(nseg + 1, 0);
  for (size_t k = 0; k < nseg; ++k) {
    const Seg& sg = segs[k];
    const mpcx_fixedbase_group_t& g = gs[sg.gi];
    for (uint32_t t = 0; t < g.nbases; ++t)
      if ((rc = h2d(l, d_in + sg.in_e[t], g.exps[t], (size_t)g.count * g.exp_words[t] * 4))) return rc;
    if (g.muls && (rc = h2d(l, d_in + sg.in_m, g.muls, (size_t)g.count * g.mul_words * 4))) return rc;
    const uint32_t* d_exps[MPCX_FB_MAX_BASES] = {d_in + sg.in_e[0], d_in + sg.in_e[1]};
    if ((rc = fixedbase_args(g, geom, di, &nwin[(size_t)sg.gi * MPCX_FB_MAX_BASES], d_exps, d_in + sg.in_m,
                             d_out + sg.out_o, &args[k])))
      return rc;
    first[k + 1] = first[k] + sg.waves;
  }
  if ((rc = h2d(l, l.stage[3].ptr, args.data(), seg_bytes)) ||
      (rc = h2d(l, (char*)l.stage[3].ptr + seg_bytes, first.data(), first_bytes)))
    return rc;
  const int ks = kstat_begin(l);
  const mpcx::FixedBaseArgs* dsegs = (const mpcx::FixedBaseArgs*)l.stage[3].ptr;
  const uint32_t* dfirst = (const uint32_t*)((const char*)l.stage[3].ptr + seg_bytes);
  hipError_t e = launch_fixedbase_multi(geom, dsegs, dfirst, (uint32_t)nseg, first[nseg],
                                        fb_split_for(dev, first[nseg]), l.st);
  if (e != hipSuccess) return hip_fail(e, "launch k_fixedbase_multi");
  dev.launches.fetch_add(1, std::memory_order_relaxed);
  double exec = 0.0;
  for (const auto& sg : segs) {
    const mpcx_fixedbase_group_t& g = gs[sg.gi];
    const FbWork w = fb_group_work(g);
    launch_log("fixedbase_multi", geom, g.count, g.fbs[0]->mod->bits, w.eb_max, w.alg);
    exec += w.exec;
  }
  kstat_end(l, ks, dev, di, "fixedbase_multi", geom, (uint32_t)total, exec);
  for (const auto& sg : segs) {  // results straight into each group's buffer
    const mpcx_fixedbase_group_t& g = gs[sg.gi];
    if ((rc = d2h(l, g.out, d_out + sg.out_o, (size_t)g.count * g.out_words * 4))) return rc;
  }
  return lane_wait(l);
}

// ------------------------------------------------------------ safe-prime sieve
namespace {
// trial-division groups: primes 59..2039 packed into products < 2^32 (the
// host sieve's grouping, csrc/host/safeprime.cpp)
struct TrialTables {
  std::vector<uint32_t> prod, start, primes;
  std::vector<uint64_t> inv;
  TrialTables() {
    std::vector<uint32_t> ps;
    for (uint32_t v = 59; v < 2048; v += 2) {
      bool pr = true;
      for (uint32_t d = 3; d * d <= v; d += 2)
        if (v % d == 0) {
          pr = false;
          break;
        }
      if (pr) ps.push_back(v);
    }
    uint64_t cur = 1;
    start.push_back(0);
    for (uint32_t p : ps) {
      if (cur * p >= (1ull << 32)) {
        prod.push_back((uint32_t)cur);
        start.push_back((uint32_t)primes.size());
        cur = 1;
      }
      cur *= p;
      primes.push_back(p);
    }
    prod.push_back((uint32_t)cur);
    start.push_back((uint32_t)primes.size());
    for (uint32_t d : prod) inv.push_back(~0ull / d);
  }
};
}  // namespace

namespace {
// One safe-prime step on lane l of device di (see mpcx_safeprime_step). With
// all_idx / all_ok non-null, also every sieve survivor's index and Fermat
// verdict (ascending index; the legacy mpcx_safeprime_sieve_fermat).
int safeprime_step_on(int di, uint64_t seed, const uint8_t* raw, uint64_t stream_off, uint32_t count, uint32_t q_bits,
                      const uint32_t* sprp_q, uint32_t n_sprp, uint32_t max_pass, uint32_t* n_sieved,
                      uint32_t* n_pass, uint32_t* pass_idx, uint32_t* pass_p, uint8_t* sprp_ok, uint32_t* all_idx,
                      uint8_t* all_ok) {
  static const TrialTables tt;
  std::unique_lock<std::mutex> lk;
  Lane& l = acquire_lane(g_devs[di], lk);
  LaneDrain drain(l);
  int rc;
  if ((rc = lane_stream(l))) return rc;
  constexpr uint32_t W = MPCX_SIEVE_MAX_BYTES / 4;
  const uint32_t nbytes = (q_bits + 7) / 8;
  Staging *sg = l.stage, *sv = l.sieve;
  const size_t ng = tt.prod.size();
  // misc buffer: survivor counter | pass counter | prod | start | primes | inv (8-byte aligned)
  const size_t off_prod = 2, off_start = off_prod + ng, off_primes = off_start + tt.start.size();
  const size_t off_inv = (off_primes + tt.primes.size() + 1) / 2 * 2;
  const size_t misc_words = off_inv + 2 * ng;
  const size_t cap = std::max<uint32_t>(count, 1);
  if ((rc = ensure_buffer(sg[0], cap * nbytes)) || (rc = ensure_buffer(sv[0], cap * W * 4)) ||
      (rc = ensure_buffer(sv[1], cap * 4)) || (rc = ensure_buffer(sv[2], misc_words * 4)) ||
      (rc = ensure_buffer(sv[3], (size_t)std::max<uint32_t>(max_pass, 1) * W * 4)) ||
      (rc = ensure_buffer(sv[4], (size_t)std::max<uint32_t>(max_pass, 1) * 4)) ||
      (rc = ensure_buffer(sv[5], (size_t)n_sprp * (W * 4 + 1) + 64)) || (all_ok && (rc = ensure_buffer(sg[3], cap))) ||
      (rc = ensure_buffer(sv[6], (cap + n_sprp) * MPCX_PRIME_L * 4)) || (rc = ensure_buffer(sv[7], (cap + n_sprp) * 8)))
    return rc;
  std::vector<uint32_t> misc(misc_words, 0);
  std::copy(tt.prod.begin(), tt.prod.end(), misc.begin() + off_prod);
  std::copy(tt.start.begin(), tt.start.end(), misc.begin() + off_start);
  std::copy(tt.primes.begin(), tt.primes.end(), misc.begin() + off_primes);
  std::memcpy(misc.data() + off_inv, tt.inv.data(), ng * 8);
  if ((rc = h2d(l, sv[2].ptr, misc.data(), misc_words * 4))) return rc;
  uint32_t* dm = (uint32_t*)sv[2].ptr;
  hipError_t e;
  if (count) {
    if (raw) {
      if ((rc = h2d(l, sg[0].ptr, raw, (size_t)count * nbytes))) return rc;
    } else {
      mpcx::DrbgArgs da{};
      da.seed = seed;
      da.off = stream_off;
      da.n = (uint64_t)count * nbytes;
      da.out = (uint8_t*)sg[0].ptr;
      e = mpcx_launch_drbg(&da, l.st);
      if (e != hipSuccess) return hip_fail(e, "launch k_drbg");
    }
    mpcx::SieveArgs sa{};
    sa.raw = (const uint8_t*)sg[0].ptr;
    sa.nbytes = nbytes;
    sa.count = count;
    sa.q_bits = q_bits;
    sa.tprod = dm + off_prod;
    sa.tstart = dm + off_start;
    sa.tprimes = dm + off_primes;
    sa.tinv = (const uint64_t*)(dm + off_inv);
    sa.ngroups = (uint32_t)ng;
    sa.out_p = (uint32_t*)sv[0].ptr;
    sa.out_idx = (uint32_t*)sv[1].ptr;
    sa.out_count = dm;
    e = mpcx_launch_sieve(&sa, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_sieve");
  }
  uint32_t* d_sq = (uint32_t*)sv[5].ptr;
  uint8_t* d_sok = (uint8_t*)(d_sq + (size_t)n_sprp * W);
  if (n_sprp && (rc = h2d(l, d_sq, sprp_q, (size_t)n_sprp * W * 4))) return rc;
  mpcx::Prime2Args pa{};
  pa.nf = (const uint32_t*)sv[0].ptr;
  pa.count_f = count;
  pa.count_dev = dm;
  pa.ok_f = all_ok ? (uint8_t*)sg[3].ptr : nullptr;
  pa.sieve_idx = (const uint32_t*)sv[1].ptr;
  pa.pass_count = dm + 1;
  pa.pass_idx = (uint32_t*)sv[4].ptr;
  pa.pass_n = (uint32_t*)sv[3].ptr;
  pa.ns = d_sq;
  pa.count_s = n_sprp;
  pa.ok_s = d_sok;
  pa.n_words = W;
  pa.r1 = (uint32_t*)sv[6].ptr;
  pa.meta = (uint32_t*)sv[7].ptr;
  if (count || n_sprp) {
    const int ks = kstat_begin(l);
    e = mpcx_launch_prime2c(pa, l.st);
    if (e != hipSuccess) return hip_fail(e, "launch k_prime2c");
    kstat_end(l, ks, g_devs[di], di, "prime2c", -1, 0, 0.0);  // work credited below from the survivor count
  }
  uint32_t cnt2[2] = {0, 0};
  if ((rc = d2h_sync(cnt2, dm, 8, l))) return rc;
  const uint32_t ns = cnt2[0], np = cnt2[1];
  if (ns > count || np > ns) return fail(MPCX_EHIP, "safe-prime step counters %u/%u out of range (%u)", ns, np, count);
  // Go-equivalent work: 2^(p-1) mod p per survivor, 2^d mod q per ride-along q
  kstat_credit("prime2c", -1, (uint64_t)ns + n_sprp,
               (double)ns * go_macs(q_bits + 1, q_bits + 1) + (double)n_sprp * go_macs(q_bits, q_bits));
  if (np > max_pass) return fail(MPCX_ENOMEM, "%u Fermat passes > max_pass %u", np, max_pass);
  std::vector<uint32_t> pidx(np), pp((size_t)np * W);
  if (np && ((rc = d2h(l, pidx.data(), sv[4].ptr, (size_t)np * 4)) || (rc = d2h(l, pp.data(), sv[3].ptr, pp.size() * 4))))
    return rc;
  if (n_sprp && (rc = d2h(l, sprp_ok, d_sok, n_sprp))) return rc;
  std::vector<uint32_t> aidx;
  std::vector<uint8_t> aok;
  if (all_ok && ns) {
    aidx.resize(ns);
    aok.resize(ns);
    if ((rc = d2h(l, aidx.data(), sv[1].ptr, (size_t)ns * 4)) || (rc = d2h(l, aok.data(), sg[3].ptr, ns))) return rc;
  }
  if ((rc = lane_wait(l))) return rc;
  // stream order
  std::vector<uint32_t> ord(np);
  for (uint32_t j = 0; j < np; ++j) ord[j] = j;
  std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return pidx[x] < pidx[y]; });
  for (uint32_t j = 0; j < np; ++j) {
    if (pass_idx) pass_idx[j] = pidx[ord[j]];
    if (pass_p) std::memcpy(pass_p + (size_t)j * W, &pp[(size_t)ord[j] * W], W * 4);
  }
  if (all_ok) {
    std::vector<uint32_t> o2(ns);
    for (uint32_t j = 0; j < ns; ++j) o2[j] = j;
    std::sort(o2.begin(), o2.end(), [&](uint32_t x, uint32_t y) { return aidx[x] < aidx[y]; });
    for (uint32_t j = 0; j < ns; ++j) {
      all_idx[j] = aidx[o2[j]];
      all_ok[j] = aok[o2[j]];
    }
  }
  if (n_sieved) *n_sieved = ns;
  if (n_pass) *n_pass = np;
  return MPCX_OK;
}
}  // namespace

int mpcx_safeprime_step(uint64_t seed, const uint8_t* raw, uint64_t stream_off, uint32_t count, uint32_t q_bits,
                        const uint32_t* sprp_q, uint32_t n_sprp, uint32_t max_pass, uint32_t* n_sieved,
                        uint32_t* n_pass, uint32_t* pass_idx, uint32_t* pass_p, uint8_t* sprp_ok) {
  if (!n_sieved || !n_pass) return fail(MPCX_EINVAL, "null counters");
  *n_sieved = *n_pass = 0;
  if (q_bits < 63 || q_bits > 1023) return fail(MPCX_EINVAL, "q_bits %u outside [63, 1023]", q_bits);
  if (count && (!pass_idx || !pass_p)) return fail(MPCX_EINVAL, "null pass buffers");
  if (n_sprp && (!sprp_q || !sprp_ok)) return fail(MPCX_EINVAL, "null strong-test buffers");
  constexpr uint32_t W = MPCX_SIEVE_MAX_BYTES / 4;
  for (uint32_t i = 0; i < n_sprp; ++i) {
    const uint32_t* qi = sprp_q + (size_t)i * W;
    if (bit_length_words(qi, W) < 3 || (qi[0] & 1u) == 0)
      return fail(MPCX_EINVAL, "strong-test candidate %u is not an odd integer >= 5", i);
  }
  if (count == 0 && n_sprp == 0) return MPCX_OK;
  return run_sliced(1, 0, [&](int di, uint32_t, uint32_t) {
    return safeprime_step_on(di, seed, raw, stream_off, count, q_bits, sprp_q, n_sprp, max_pass, n_sieved, n_pass,
                             pass_idx, pass_p, sprp_ok, nullptr, nullptr);
  });
}

int mpcx_safeprime_sieve_fermat(const uint8_t* raw, uint32_t nbytes, uint32_t count, uint32_t q_bits,
                                uint32_t* n_out, uint32_t* idx_out, uint8_t* ok_out) {
  if (!n_out) return fail(MPCX_EINVAL, "null n_out");
  *n_out = 0;
  if (q_bits < 63 || q_bits > 1023) return fail(MPCX_EINVAL, "q_bits %u outside [63, 1023]", q_bits);
  if (nbytes != (q_bits + 7) / 8) return fail(MPCX_EINVAL, "nbytes %u != (q_bits + 7) / 8", nbytes);
  if (count == 0) return MPCX_OK;
  if (!raw || !idx_out || !ok_out) return fail(MPCX_EINVAL, "null buffer");
  return run_sliced(1, 0, [&](int di, uint32_t, uint32_t) {
    uint32_t np = 0;
    std::vector<uint32_t> pidx(count);
    std::vector<uint32_t> pp((size_t)count * (MPCX_SIEVE_MAX_BYTES / 4));
    return safeprime_step_on(di, 0, raw, 0, count, q_bits, nullptr, 0, count, n_out, &np, pidx.data(), pp.data(),
                             nullptr, idx_out, ok_out);
  });
}
