// api.hip — the C-ABI of include/albatross_amd.h.
//
// Host-side orchestration only: uploads POD feature vectors, enqueues the HIP
// kernels of gram.hip / chol.hip / gemm.hip / reduce.hip on the context's
// stream, reads back the small results.  No CPU arithmetic fallback exists.
// The batched fits (agp_nll_batch, agp_fit_create_batch) are built on the front end of batch_front.h, their
// workspaces - and agp_nll's - on the layouts of batch_layout.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <chrono>
#include <cstdio>
#include <new>
#include <thread>

#include "api_internal.h"
#include "batch_front.h"
#include <deque>
#include <mutex>
#include <tuple>
#include <unordered_map>
#include "trace.h"
#include "pub.h"

namespace agp {

long long round_up(long long x, long long m) { return (x + m - 1) / m * m; }

// leading dimension of the factor: even (16-B aligned columns) and not a
// multiple of 256 doubles, so that consecutive columns do not alias the same
// HBM channel / L2 set pattern
long long factor_ld(long long n) {
  long long ld = round_up(n, 8);
  if (ld % 256 == 0) ld += 8;
  return ld;
}

}  // namespace agp

using namespace agp;

static agp_context_ext *ext_of(agp_context *ctx) { return &static_cast<agp_context_impl *>(ctx)->ext; }
std::atomic<unsigned long long> g_kernel_uid{1};

namespace agp {
namespace {
constexpr size_t DEV_CACHE_BYTES = 8ull << 30;
struct DevCache {
  std::mutex mu;
  std::unordered_map<void *, std::pair<int, size_t>> live;   // blocks handed out: device, size
  std::deque<std::tuple<int, size_t, void *>> parked;        // oldest first
  size_t held = 0;
};
DevCache &dev_cache() {
  // never destroyed: contexts held in a host program's statics are closed after this library's statics would be gone
  static DevCache *c = new DevCache();
  return *c;
}
}  // namespace

int dev_malloc_plain_bytes(void **p, size_t bytes) { return hipMalloc(p, bytes); }

int dev_malloc_bytes(void **p, size_t bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  DevCache &c = dev_cache();
  {
    std::lock_guard<std::mutex> lock(c.mu);
    for (auto it = c.parked.begin(); it != c.parked.end(); ++it)
      if (std::get<0>(*it) == dev && std::get<1>(*it) == bytes) {
        *p = std::get<2>(*it);
        c.held -= bytes;
        c.parked.erase(it);
        c.live[*p] = {dev, bytes};
        return hipSuccess;
      }
  }
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lock(c.mu);
    c.live[*p] = {dev, bytes};
  } else {
    dev_cache_trim();  // out of memory with blocks parked: give them back and try once more
    const hipError_t e2 = hipMalloc(p, bytes);
    if (e2 == hipSuccess) {
      std::lock_guard<std::mutex> lock(c.mu);
      c.live[*p] = {dev, bytes};
    }
    return e2;
  }
  return e;
}

int dev_free(void *p) {
  if (!p) return hipSuccess;
  DevCache &c = dev_cache();
  std::pair<int, size_t> info{-1, 0};
  {
    std::lock_guard<std::mutex> lock(c.mu);
    auto it = c.live.find(p);
    if (it != c.live.end()) { info = it->second; c.live.erase(it); }
  }
  if (info.first < 0 || info.second > DEV_CACHE_BYTES / 4) return hipFree(p);
  (void)hipDeviceSynchronize();  // what hipFree implies: nothing in flight uses the block any more
  std::vector<void *> evict;
  {
    std::lock_guard<std::mutex> lock(c.mu);
    c.parked.emplace_back(info.first, info.second, p);
    c.held += info.second;
    while (c.held > DEV_CACHE_BYTES || c.parked.size() > 96) {
      evict.push_back(std::get<2>(c.parked.front()));
      c.held -= std::get<1>(c.parked.front());
      c.parked.pop_front();
    }
  }
  for (void *q : evict) (void)hipFree(q);
  return hipSuccess;
}

// hipFree of a block that MAY have come from dev_malloc (a factor parked in a context pool, a buffer handed from one
// owner to another): the `live` entry goes with it - a stale entry would later match an unrelated hipMalloc that
// happens to return the same address, and dev_free would park that block under the old (larger) size.
int dev_release(void *p) {
  if (!p) return hipSuccess;
  DevCache &c = dev_cache();
  {
    std::lock_guard<std::mutex> lock(c.mu);
    c.live.erase(p);
  }
  return hipFree(p);
}

// A block of dev_malloc that moves into a context slot (ParkSlot) stops being this table's: the slot frees through
// dev_release or hands the block to whoever takes it next, and that may be the OTHER image of the library in a process that
// loads both (the tests: libalbatross_amd.so and libalbatross_amd_debug.so each have a table, the context and its slots
// are one).  An entry left behind would outlive a hipFree made by that image and match the next block at the address.
void dev_forget(void *p) {
  if (!p) return;
  DevCache &c = dev_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  c.live.erase(p);
}

void dev_cache_trim() {
  DevCache &c = dev_cache();
  std::vector<void *> all;
  {
    std::lock_guard<std::mutex> lock(c.mu);
    for (auto &t : c.parked) all.push_back(std::get<2>(t));
    c.parked.clear();
    c.held = 0;
  }
  for (void *q : all) (void)hipFree(q);
}
}  // namespace agp

namespace agp {
// the Gram launchers have no context: they follow the switches of the context created last
static bool g_gram_sop = true;
bool gram_sop_enabled() { return g_gram_sop; }
// (libalbatross_amd_debug.so holds its own copy of this static, which no agp_context_create of the product library sets: its
// Gram entry points set it to the switch of the context they are handed for the length of their launch and put it back -
// debug_api.hip: GramSopScope)
void gram_sop_set(bool on) { g_gram_sop = on; }
}  // namespace agp

extern "C" {

const char *agp_status_string(int status) {
  switch (status) {
  case AGP_OK: return "ok";
  case AGP_ERR_INVALID_ARGUMENT: return "invalid argument";
  case AGP_ERR_NAN_INPUT: return "covariance matrix contains NaN";
  case AGP_ERR_NOT_POSITIVE_DEFINITE: return "covariance matrix is not positive definite";
  case AGP_ERR_HIP: return "HIP runtime error";
  case AGP_ERR_COMM: return "communication error";
  case AGP_ERR_UNSUPPORTED: return "unsupported";
  case AGP_ERR_NO_DEVICE: return "no HIP device";
  case AGP_ERR_NOT_CONVERGED: return "iterative solve did not converge";
  default: return "unknown status";
  }
}

int agp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static constexpr long long BACKSUB_COOP_MAX_N = 2047;
// the switches of include/albatross_amd.h ("switches"): read here, once per context, and nowhere else; they take effect
// through ctx->tune alone, so a context keeps the settings it was created under (the one exception: AGP_GRAM_SOP, above)
static agp_context::Tuning read_tuning() {
  agp_context::Tuning t;
  auto flag = [](const char *name, bool dflt) {
    const char *e = getenv(name);
    return e && e[0] ? e[0] == '1' : dflt;
  };
  auto number = [](const char *name, long long dflt) {
    const char *e = getenv(name);
    return e && e[0] ? atoll(e) : dflt;
  };
  t.panel_fused = flag("AGP_PANEL_FUSED", true);
  t.step_below = number("AGP_STEP_BELOW", 4608);
  t.gram_sop = flag("AGP_GRAM_SOP", true);
  t.backsub_coop = flag("AGP_BACKSUB_COOP", true);
  t.backsub_coop_max = number("AGP_BACKSUB_COOP_MAX", BACKSUB_COOP_MAX_N);
  t.mixed_bf16 = flag("AGP_MIXED_BF16", true);
  t.mixed_f16 = flag("AGP_MIXED_F16", true);
  t.f16x2.lds_pad = (int)number("AGP_F16X2_LDS_PAD", 8192);
  t.f16x2.terms = number("AGP_F16X2_TERMS", 4) == 3 ? 3 : 4;
  t.f16x2.chunk = number("AGP_F16X2_CHUNK", 32) == 64 ? 64 : 32;
  t.mixed_nbo = number("AGP_MIXED_NBO", 512);
  t.fp64_nbo = number("AGP_FP64_NBO", 0);
  // (the rule agp_fit_create_mixed applies to AGP_MIXED_NBO: outer block edges must fall on 128-column panel edges, and
  // only a width above 512 changes anything - the panels of an outer block are NB = 128 wide, and a 700-wide block would
  // end inside its last panel)
  if (t.fp64_nbo <= 512 || t.fp64_nbo % 128 != 0) t.fp64_nbo = 0;
  t.bf16x3.lds_pad = (int)number("AGP_BF16X3_LDS_PAD", 8192);
  t.sparse_pivoted = flag("AGP_SPARSE_PIVOTED", false);
  t.predict_chunk = number("AGP_PREDICT_CHUNK", 0);
  t.shard_block = number("AGP_SHARD_BLOCK", 0);
  t.shard_force_comm = flag("AGP_SHARD_FORCE_COMM", false);
  t.shard_host_pacing = flag("AGP_SHARD_HOST_PACING", false);
  if (const char *e = getenv("AGP_SHARD_MASK_GFLOP")) t.shard_mask_gflop = atof(e);
  t.merge_above = number("AGP_MERGE_ABOVE", 8704);
  return t;
}

// everything of agp_context_create that can fail: the caller destroys the context then
static int context_init(agp_context_impl *ctx, int device_id) {
  AGP_HIP_CHECK(ctx, hipSetDevice(device_id));
  {
    // main / panel stream at the highest priority: its short kernels must not
    // queue behind the bulk update running on stream2
    int lo = 0, hi = 0;
    AGP_HIP_CHECK(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
    AGP_HIP_CHECK(ctx, hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, hi));
    AGP_HIP_CHECK(ctx, hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, lo));
    // (no further streams in the context: one more high-priority stream changed how the runtime maps streams onto its few
    // hardware queues and cost 3.5 ms per N = 16384 fit before it was used at all)
    AGP_HIP_CHECK(ctx, hipStreamCreateWithPriority(&ctx->stream3, hipStreamNonBlocking, lo));
    AGP_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_inv, hipEventDisableTiming));
    AGP_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_c, hipEventDisableTiming));
    // CU mask of the end-phase bulk stream: bit i = CU i, and CU i sits on XCD i % 8 (measured with
    // scripts/probe_cumask.py: dropping the LAST indices keeps the XCDs balanced, dropping i % 32 >= 28 does not).
    // AGP_MASK_CUS = CUs the bulk stream keeps (multiple of 8; 0 = no masked stream)
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id);
    ctx->cus = cus;
    // 224 of 256 CUs (28 per XCD) from 8704 remaining rows on is the best pair at N = 16384 (profiles/r02/sweep_mask.txt)
    const int keep = cus / 8 * 7 / 8 * 8;
    if (keep > 0 && keep < cus) {
      uint32_t mask[16] = {0};
      for (int i = 0; i < keep && i < 512; ++i) mask[i / 32] |= 1u << (i % 32);
      if (hipExtStreamCreateWithCUMask(&ctx->stream_masked, (uint32_t)((cus + 31) / 32), mask) != hipSuccess) {
        (void)hipGetLastError();
        ctx->stream_masked = nullptr;
      }
    }
  }
  AGP_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_a, hipEventDisableTiming));
  AGP_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_b, hipEventDisableTiming));
  // flags and scalars of a factorisation: ONE block on either side ([4 ints | 4 doubles]) so that one 48-byte copy brings both back
  AGP_HIP_CHECK(ctx, ctx->d_headcnt.alloc_plain(sizeof(unsigned long long) * agp_context::HEADCNT_WORDS));
  AGP_HIP_CHECK(ctx, ctx->d_flags.alloc_plain(4 * sizeof(int) + 4 * sizeof(double)));
  ctx->d_scalars = reinterpret_cast<double *>(ctx->d_flags + 4);
  AGP_HIP_CHECK(ctx, hipHostMalloc(&ctx->h_flags, 4 * sizeof(int) + 4 * sizeof(double)));
  ctx->h_scalars = reinterpret_cast<double *>(ctx->h_flags + 4);
  if (hipHostGetDevicePointer(&ctx->h_status_dev, ctx->h_flags, 0) != hipSuccess) { (void)hipGetLastError(); ctx->h_status_dev = nullptr; }
  for (auto &e : ctx->stage_ev) AGP_HIP_CHECK(ctx, hipEventCreate(&e));
  for (auto &sl : ctx->ext.slots) AGP_HIP_CHECK(ctx, sl.dev.alloc_plain(sizeof(DevProgram)));
  return AGP_OK;
}

int agp_context_create(int device_id, agp_context **out) {
  if (!out) return AGP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AGP_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= n) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = new (std::nothrow) agp_context_impl();
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  ctx->device = device_id;
  ctx->tune = read_tuning();
  agp::g_gram_sop = ctx->tune.gram_sop;
  const int st = context_init(ctx, device_id);
  if (st != AGP_OK) {
    agp_context_destroy(ctx);
    return st;
  }
  *out = ctx;
  return AGP_OK;
}

void agp_context_destroy(agp_context *c) {
  if (!c) return;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (agp_context *h : ctx->helpers) agp_context_destroy(h);
  ctx->helpers.clear();
  for (auto e : ctx->gemm_events) (void)hipEventDestroy(e);
  for (auto e : ctx->stage_ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  if (ctx->h_flags) (void)hipHostFree(ctx->h_flags);
  if (ctx->ev_a) (void)hipEventDestroy(ctx->ev_a);
  if (ctx->ev_b) (void)hipEventDestroy(ctx->ev_b);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
  if (ctx->ev_inv) (void)hipEventDestroy(ctx->ev_inv);
  if (ctx->stream_masked) (void)hipStreamDestroy(ctx->stream_masked);
  if (ctx->stream_comm) (void)hipStreamDestroy(ctx->stream_comm);
  if (ctx->ev_c) (void)hipEventDestroy(ctx->ev_c);
  delete ctx;  // (its device memory goes with its members: dev_mem.h)
  agp::dev_cache_trim();  // (the parked blocks of dev_free: a process that closes its contexts gives its device memory back)
}

int agp_context_synchronize(agp_context *ctx) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AGP_HIP_CHECK(ctx, hipDeviceSynchronize());
  return AGP_OK;
}

// device buffers for AGP_DEVICE arguments (include/albatross_amd.h, "device memory"): plain runtime calls on the context's
// device, so that a host program needs neither HIP headers nor a second runtime in its process
int agp_device_malloc(agp_context *ctx, int64_t bytes, void **out) {
  if (!ctx || !out || bytes <= 0) return AGP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AGP_HIP_CHECK(ctx, hipMalloc(out, (size_t)bytes));
  return AGP_OK;
}

int agp_device_free(agp_context *ctx, void *ptr) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  if (!ptr) return AGP_OK;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  AGP_HIP_CHECK(ctx, hipFree(ptr));
  return AGP_OK;
}

int agp_memcpy(agp_context *ctx, void *dst, const void *src, int64_t bytes, int kind) {
  if (!ctx || bytes < 0 || (kind != AGP_HOST && kind != AGP_DEVICE) || (bytes > 0 && (!dst || !src))) return AGP_ERR_INVALID_ARGUMENT;
  if (bytes == 0) return AGP_OK;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (kind == AGP_HOST) AGP_HIP_CHECK(ctx, hipDeviceSynchronize());  // the context's streams are non-blocking: the copy would not wait for them
  AGP_HIP_CHECK(ctx, hipMemcpy(dst, src, (size_t)bytes, kind == AGP_DEVICE ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
  return AGP_OK;
}

const char *agp_last_error(const agp_context *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int agp_set_profiling(agp_context *ctx, int enabled) {
  if (!ctx) return AGP_ERR_INVALID_ARGUMENT;
  ctx->profiling = enabled != 0;
  return AGP_OK;
}

int agp_last_stage_ms(const agp_context *c, int stage, double *ms) {
  if (!c || !ms || stage < 0 || stage > 14) return AGP_ERR_INVALID_ARGUMENT;
  *ms = c->stage_ms[stage];
  return AGP_OK;
}


// ---- covariance function ---------------------------------------------------
int agp_kernel_create(const agp_kernel_node *postfix, int n_nodes, agp_kernel **out) {
  if (!postfix || !out || n_nodes <= 0 || n_nodes > AGP_MAX_KERNEL_NODES) return AGP_ERR_INVALID_ARGUMENT;
  int depth = 0, mask = 0, uses_eq = 0;
  for (int t = 0; t < n_nodes; ++t) {
    const agp_kernel_node &nd = postfix[t];
    switch (nd.op) {
    case AGP_OP_SQUARED_EXPONENTIAL:
    case AGP_OP_EXPONENTIAL:
    case AGP_OP_MATERN32:
    case AGP_OP_MATERN52:
      if (nd.metric < 0 || nd.metric > AGP_METRIC_ANGULAR) return AGP_ERR_INVALID_ARGUMENT;
      mask |= 1 << nd.metric;
      ++depth;
      break;
    case AGP_OP_CONSTANT: ++depth; break;
    case AGP_OP_INDEPENDENT_NOISE:
    case AGP_OP_NUGGET: uses_eq = 1; ++depth; break;
    case AGP_OP_POLYNOMIAL:
      if (nd.order < 0 || nd.order > 3) return AGP_ERR_UNSUPPORTED;
      ++depth;
      break;
    case AGP_OP_SCALING:
      if (nd.column < 0 || nd.column >= AGP_MAX_SCALE_COLUMNS) return AGP_ERR_INVALID_ARGUMENT;
      ++depth;
      break;
    case AGP_OP_SUM:
    case AGP_OP_PRODUCT:
      if (depth < 2) return AGP_ERR_INVALID_ARGUMENT;
      --depth;
      break;
    case AGP_OP_MEASUREMENT_ONLY:
      if (depth < 1) return AGP_ERR_INVALID_ARGUMENT;
      break;
    case AGP_OP_TYPE_PAIR:
      if (depth < 1 || nd.column < 0 || nd.column >= AGP_MAX_SCALE_COLUMNS) return AGP_ERR_INVALID_ARGUMENT;
      break;
    default: return AGP_ERR_INVALID_ARGUMENT;
    }
    if (depth > AGP_MAX_STACK) return AGP_ERR_UNSUPPORTED;
  }
  if (depth != 1) return AGP_ERR_INVALID_ARGUMENT;
  agp_kernel_full *k = new (std::nothrow) agp_kernel_full();
  if (!k) return AGP_ERR_INVALID_ARGUMENT;
  std::memset(&k->prog, 0, sizeof(k->prog));
  k->prog.n_nodes = n_nodes;
  k->prog.metric_mask = mask;
  k->prog.uses_equality = uses_eq;
  std::memcpy(k->prog.nodes, postfix, sizeof(agp_kernel_node) * (size_t)n_nodes);
  k->uid = g_kernel_uid.fetch_add(1);
  *out = k;
  return AGP_OK;
}

void agp_kernel_destroy(agp_kernel *k) { delete static_cast<agp_kernel_full *>(k); }

}  // extern "C"

// device copy of a kernel program (small LRU ring per context)
int device_program(agp_context *ctx, const agp_kernel *k, const DevProgram **out) {
  agp_context_ext *x = ext_of(ctx);
  const unsigned long long uid = static_cast<const agp_kernel_full *>(k)->uid;
  for (auto &sl : x->slots)
    if (sl.uid == uid) {
      *out = sl.dev;
      return AGP_OK;
    }
  ProgSlot &sl = x->slots[x->next];
  x->next = (x->next + 1) % 8;
  // the slot may still be read by kernels in flight on the stream
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, hipMemcpy(sl.dev, &k->prog, sizeof(DevProgram), hipMemcpyHostToDevice));
  sl.uid = uid;
  *out = sl.dev;
  return AGP_OK;
}

namespace agp {
int device_program_for(agp_context *ctx, const agp_kernel *k, const DevProgram **out) {
  return device_program(ctx, k, out);
}
}  // namespace agp

int validate_features(const agp_features *f) {
  if (!f || f->n < 0 || f->dim < 1 || f->dim > AGP_MAX_DIM) return AGP_ERR_INVALID_ARGUMENT;
  if (f->n_scale_columns < 0 || f->n_scale_columns > AGP_MAX_SCALE_COLUMNS) return AGP_ERR_INVALID_ARGUMENT;
  if (f->n > 0 && !f->coords) return AGP_ERR_INVALID_ARGUMENT;
  if (f->n_scale_columns > 0 && f->n > 0 && !f->scales) return AGP_ERR_INVALID_ARGUMENT;
  return AGP_OK;
}

// Make a device view of a feature vector (uploads host data; `copy` forces an
// owned device copy of device-resident data as well).
int to_device(agp_context *ctx, const agp_features *f, bool copy, DeviceFeatures *out) {
  const int st = validate_features(f);
  if (st != AGP_OK) return st;
  out->release();
  FeatView v;
  v.n = f->n; v.dim = f->dim; v.nsc = f->n_scale_columns; v.meas = f->is_measurement;
  v.coords = nullptr; v.ids = nullptr; v.scales = nullptr;
  const bool on_host = f->location == AGP_HOST;
  const hipMemcpyKind kind = on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (f->n > 0) {
    if (on_host || copy) {
      const size_t cb = sizeof(double) * (size_t)f->n * (size_t)f->dim;
      AGP_HIP_CHECK(ctx, out->owned[0].alloc_plain(cb));
      AGP_HIP_CHECK(ctx, hipMemcpyAsync(out->owned[0], f->coords, cb, kind, ctx->stream));
      v.coords = static_cast<const double *>(out->owned[0].get());
      if (f->eq_id) {
        const size_t ib = sizeof(long long) * (size_t)f->n;
        AGP_HIP_CHECK(ctx, out->owned[1].alloc_plain(ib));
        AGP_HIP_CHECK(ctx, hipMemcpyAsync(out->owned[1], f->eq_id, ib, kind, ctx->stream));
        v.ids = static_cast<const long long *>(out->owned[1].get());
      }
      if (f->n_scale_columns > 0) {
        const size_t sb = sizeof(double) * (size_t)f->n * (size_t)f->n_scale_columns;
        AGP_HIP_CHECK(ctx, out->owned[2].alloc_plain(sb));
        AGP_HIP_CHECK(ctx, hipMemcpyAsync(out->owned[2], f->scales, sb, kind, ctx->stream));
        v.scales = static_cast<const double *>(out->owned[2].get());
      }
      if (on_host) AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // pageable source
    } else {
      v.coords = f->coords;
      v.ids = reinterpret_cast<const long long *>(f->eq_id);
      v.scales = f->n_scale_columns > 0 ? f->scales : nullptr;
    }
  }
  out->v = v;
  return AGP_OK;
}

namespace agp {
int features_to_device(agp_context *ctx, const agp_features *f, bool copy, DeviceFeatures *out) {
  return to_device(ctx, f, copy, out);
}
}  // namespace agp

int reserve_ws(agp_context *ctx, GrowBuf<double> &ws, size_t need) {
  if (ws.bytes() >= need) return AGP_OK;
  if (ws) AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  AGP_HIP_CHECK(ctx, ws.reserve(need));
  return AGP_OK;
}

// a device staging copy of an n-vector living at `location`
int vector_to_device(agp_context *ctx, const double *src, long long n, int location, double *dst) {
  const hipMemcpyKind kind = location == AGP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, kind, ctx->stream));
  if (location == AGP_HOST) AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

int copy_out(agp_context *ctx, const double *dev, long long count, double *dst, int location) {
  const hipMemcpyKind kind = location == AGP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(dst, dev, sizeof(double) * (size_t)count, kind, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

int copy_out_2d(agp_context *ctx, const double *dev, long long ld_dev, long long rows, long long cols,
                       double *dst, long long ld_dst, int location) {
  if (location == AGP_HOST && ld_dev == ld_dst) {  // one contiguous transfer instead of one per column
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(dst, dev, sizeof(double) * ((size_t)ld_dev * (size_t)(cols - 1) + (size_t)rows),
                                      hipMemcpyDeviceToHost, ctx->stream));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return AGP_OK;
  }
  if (location == AGP_HOST && (size_t)rows * (size_t)cols >= (1u << 16)) {
    // re-pitch on the device, then one contiguous transfer
    DevMem<double> tmp;
    const size_t elems = (size_t)ld_dst * (size_t)(cols - 1) + (size_t)rows;
    AGP_HIP_CHECK(ctx, tmp.alloc_plain(sizeof(double) * elems));
    hipError_t e = hipMemcpy2DAsync(tmp, sizeof(double) * (size_t)ld_dst, dev, sizeof(double) * (size_t)ld_dev,
                                    sizeof(double) * (size_t)rows, (size_t)cols, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, tmp, sizeof(double) * elems, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    tmp.reset();
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return AGP_ERR_HIP; }
    return AGP_OK;
  }
  const hipMemcpyKind kind = location == AGP_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, sizeof(double) * (size_t)ld_dst, dev, sizeof(double) * (size_t)ld_dev,
                                      sizeof(double) * (size_t)rows, (size_t)cols, kind, ctx->stream));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return AGP_OK;
}

// Gram + diag add + LL^T (+ fused forward substitution) on A / y.  On return
// the stream has been synchronised and ctx->h_flags / h_scalars are valid.
// finish = false: everything is enqueued, nothing is waited for - the caller goes on enqueueing (the backward
// substitution of a fit) and calls finish_factor() after its own synchronisation.
static void finish_factor(agp_context_impl *ctx, const FactorTimers &timers) {
  if (!ctx->profiling) return;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ctx->stage_ev[0], ctx->stage_ev[1]);
  ctx->stage_ms[0] = ms;
  (void)hipEventElapsedTime(&ms, ctx->stage_ev[1], ctx->stage_ev[2]);
  ctx->stage_ms[1] = ms;
  double sum = 0., flop = 0.;
  for (int i = 0; i + 1 < timers.used; i += 2) {
    (void)hipEventElapsedTime(&ms, timers.ev[i], timers.ev[i + 1]);
    sum += ms;
    flop += timers.flops[i / 2];
  }
  ctx->stage_ms[3] = sum;
  ctx->stage_ms[4] = timers.used / 2;
  ctx->stage_ms[5] = flop;  // flop of the trailing updates (not ms)
}

static constexpr size_t STATUS_BYTES = 4 * sizeof(int) + 4 * sizeof(double);

// pre (optional): fills and copies the caller wants made BEFORE the Gram matrix is built, in the same launch as the
// zeroing of the flags and the sentinel fills of the panel kernels (pub.h: a fit of a few hundred points used to
// spend ten launches on these)
// req: what the caller asks of the factorisation (its prep and timers are filled in here); outcome (optional): what
// factor_lower reported
static int build_and_factor(agp_context *c, const DevProgram *dprog, const DevProgram *hprog, const FeatView &xm,
                            double *A, long long lda, double *invd, double *y, const double *yvar, bool finish = true,
                            FactorTimers *timers_out = nullptr, PrepArgs *pre = nullptr, bool copy_status = true,
                            const double *gram_copy = nullptr, FactorRequest req = {}, FactorOutcome *outcome = nullptr) {
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  const long long n = xm.n;
  hipStream_t s = ctx->stream;
  {
    PrepArgs local;
    PrepArgs *prep = pre ? pre : &local;
    prep->fill(ctx->d_flags, 0ull, (long long)(STATUS_BYTES / 8));
    if (prep->n + 5 <= PREP_MAX) req.prep = panel_fused_plan(ctx, invd, 0, n, true, prep);
    launch_prep(s, *prep);
  }
  const bool prof = ctx->profiling;
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[0], s));
  // as_measurements(features) -> covariance_function_(measurement_features)   gp.hpp:288-290
  {
    TraceRange tr("agp: gram (compute_covariance_matrix, callers.hpp:107-166)");
    // (gram_copy: the caller holds this very matrix - same leading dimension, measurement variances included - already)
    if (gram_copy) launch_copy_lower(s, gram_copy, lda, n, A, ctx->d_flags);
    else launch_gram(s, dprog, xm, xm, /*symmetric=*/true, /*lower_only=*/true, A, lda, yvar, ctx->d_flags, hprog);
  }
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[1], s));
  TraceRange tr_factor("agp: factor LL^T + forward substitution (SerializableLDLT, serializable_ldlt.hpp:27)");
  FactorTimers timers;
  if (prof) {
    const size_t want = (size_t)(2 * (2 * ((n + NB - 1) / NB) + 4));
    while (ctx->gemm_events.size() < want) {
      hipEvent_t e;
      AGP_HIP_CHECK(ctx, hipEventCreate(&e));
      ctx->gemm_events.push_back(e);
    }
    ctx->gemm_flops.assign(want / 2, 0.);
    timers.ev = ctx->gemm_events.data();
    timers.flops = ctx->gemm_flops.data();
    timers.n_ev = (int)want;
  }
  req.timers = prof ? &timers : nullptr;
  const FactorOutcome done = factor_lower(ctx, A, n, lda, invd, y, req);
  if (outcome) *outcome = done;
  if (prof) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[2], s));
  // (copy_status false: the caller's next launch forwards the status block itself - backsub_coop_kernel)
  if (copy_status || finish) AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_flags, ctx->d_flags, STATUS_BYTES, hipMemcpyDeviceToHost, s));
  if (timers_out) *timers_out = timers;
  if (!finish) return AGP_OK;
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  finish_factor(ctx, timers);
  return AGP_OK;
}

namespace agp {
// build_and_factor as agp_nll calls it, for the gradient (gradient.hip)
int build_and_factor_nll(agp_context *c, const DevProgram *dprog, const DevProgram *hprog, const FeatView &xm, double *A,
                         long long lda, double *invd, double *y, const double *yvar) {
  return build_and_factor(c, dprog, hprog, xm, A, lda, invd, y, yvar);
}
}  // namespace agp

int status_from_flags(const agp_context *ctx) {
  if (ctx->h_flags[2]) {  // a consumer of the fused panel kernel gave up waiting for its producer (chol.hip)
    const_cast<agp_context *>(ctx)->last_error = "panel kernel: hand-over of a diagonal block timed out";
    return AGP_ERR_HIP;
  }
  if (ctx->h_flags[0]) return AGP_ERR_NAN_INPUT;
  if (ctx->h_flags[1]) return AGP_ERR_NOT_POSITIVE_DEFINITE;
  return AGP_OK;
}

extern "C" {

// ---- Gram ------------------------------------------------------------------
int agp_gram(agp_context *ctx, const agp_kernel *k, const agp_features *x, const agp_features *y, double *out,
             int64_t ld, int out_location) {
  if (!ctx || !k || !x || !out) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  if (y && (st = validate_features(y)) != AGP_OK) return st;
  if (y && y->dim != x->dim) return AGP_ERR_INVALID_ARGUMENT;
  const long long rows = x->n, cols = y ? y->n : x->n;
  if (rows == 0 || cols == 0) return AGP_OK;
  if (ld < rows) return AGP_ERR_INVALID_ARGUMENT;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx, dy;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  if (y && (st = to_device(ctx, y, false, &dy)) != AGP_OK) { dx.release(); return st; }
  const FeatView &vy = y ? dy.v : dx.v;
  if (out_location == AGP_DEVICE) {
    launch_gram(ctx->stream, dprog, dx.v, vy, y == nullptr, false, out, ld, nullptr, nullptr, &k->prog);
    st = AGP_OK;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); st = AGP_ERR_HIP; }
  } else {
    const long long ldd = round_up(rows, 2);
    st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (size_t)ldd * (size_t)cols);
    if (st == AGP_OK) {
      launch_gram(ctx->stream, dprog, dx.v, vy, y == nullptr, false, ctx->ws_aux, ldd, nullptr, nullptr, &k->prog);
      st = copy_out_2d(ctx, ctx->ws_aux, ldd, rows, cols, out, ld, AGP_HOST);
    }
  }
  dx.release();
  dy.release();
  return st;
}

// ---- Gram of LinearCombination features ------------------------------------------------------------------
int agp_gram_combined(agp_context *ctx, const agp_kernel *k, const agp_features *x, int64_t nx, const int64_t *x_offsets,
                      const double *x_coefficients, const agp_features *y, int64_t ny, const int64_t *y_offsets,
                      const double *y_coefficients, double *out, int64_t ld, int out_location) {
  if (!ctx || !k || !x || !out || nx < 0 || ny < 0) return AGP_ERR_INVALID_ARGUMENT;
  if ((x_offsets == nullptr) != (x_coefficients == nullptr) || (y_offsets == nullptr) != (y_coefficients == nullptr))
    return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  if (y && (st = validate_features(y)) != AGP_OK) return st;
  if (y && y->dim != x->dim) return AGP_ERR_INVALID_ARGUMENT;
  const bool symmetric = y == nullptr;
  const long long ex = x->n, ey = y ? y->n : x->n;
  const long long na = x_offsets ? nx : ex, nb = symmetric ? na : (y_offsets ? ny : ey);
  if (na == 0 || nb == 0) return AGP_OK;
  if (ld < na) return AGP_ERR_INVALID_ARGUMENT;
  if (x_offsets && (x_offsets[0] != 0 || x_offsets[nx] != ex)) return AGP_ERR_INVALID_ARGUMENT;
  if (!symmetric && y_offsets && (y_offsets[0] != 0 || y_offsets[ny] != ey)) return AGP_ERR_INVALID_ARGUMENT;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dx, dy;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  if (y && (st = to_device(ctx, y, false, &dy)) != AGP_OK) return st;
  const FeatView &vy = y ? dy.v : dx.v;
  // workspace: expanded Gram | contracted result | offsets / coefficients of both sides
  const long long ldk = round_up(ex, 2), ldo = round_up(na, 2);
  const size_t k_elems = (size_t)ldk * (size_t)ey, o_elems = (size_t)ldo * (size_t)nb;
  const size_t meta = (size_t)(x_offsets ? 2 * (nx + 1) + ex : 0) + (size_t)((!symmetric && y_offsets) ? 2 * (ny + 1) + ey : 0) + 8;
  if ((st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (k_elems + o_elems + meta))) != AGP_OK) return st;
  double *Kd = ctx->ws_aux, *Od = Kd + k_elems, *m = Od + o_elems;
  hipStream_t s = ctx->stream;
  const long long *xoff_d = nullptr, *yoff_d = nullptr;
  const double *xc_d = nullptr, *yc_d = nullptr;
  if (x_offsets) {
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(m, x_offsets, sizeof(int64_t) * (size_t)(nx + 1), hipMemcpyHostToDevice, s));
    xoff_d = reinterpret_cast<const long long *>(m);
    m += nx + 1;
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(m, x_coefficients, sizeof(double) * (size_t)ex, hipMemcpyHostToDevice, s));
    xc_d = m;
    m += ex;
  }
  if (symmetric) { yoff_d = xoff_d; yc_d = xc_d; }
  else if (y_offsets) {
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(m, y_offsets, sizeof(int64_t) * (size_t)(ny + 1), hipMemcpyHostToDevice, s));
    yoff_d = reinterpret_cast<const long long *>(m);
    m += ny + 1;
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(m, y_coefficients, sizeof(double) * (size_t)ey, hipMemcpyHostToDevice, s));
    yc_d = m;
  }
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));  // pageable sources
  launch_gram(s, dprog, dx.v, vy, symmetric, false, Kd, ldk, nullptr, nullptr, &k->prog);
  launch_contract_combinations(s, Kd, ldk, xoff_d, xc_d, na, yoff_d, yc_d, nb, symmetric, Od, ldo);
  return copy_out_2d(ctx, Od, ldo, na, nb, out, ld, out_location);
}

// ---- fit -------------------------------------------------------------------
void agp_fit_destroy(agp_fit *fit) {
  if (!fit) return;
  (void)hipSetDevice(fit->device);
  agp_context *ctx = fit->ctx;
  // What the fit owns is offered to the context's slots, where the next fit of the same size finds it (kernels reading
  // the blocks were enqueued on the context's streams; their next user is enqueued on the same streams, after them).  The
  // most recent size wins a slot: a buffer of another size parked there - the headline's 2 GiB factor, say, in a process
  // that goes on to fit 512 points - would cost every later fit a hipMalloc and a hipFree: +0.2 ms per N = 512 fit, the
  // "0.21 vs 0.41 ms" of the round-4 review.  What a slot refuses goes with its owner.
  if (fit->slab && --fit->slab->refs == 0) {
    if (ctx && ctx->pool_batch.park(fit->slab->base, fit->slab->bytes)) (void)fit->slab->base.release();
    delete fit->slab;
  }
  // (agp_factor_create takes its factor from dev_malloc: what the slot keeps is forgotten by the table of live blocks)
  if (ctx && fit->own_A && ctx->pool_A.park(fit->own_A, fit->A_bytes)) dev_forget(fit->own_A.release());
  if (ctx && fit->aux_base && ctx->pool_aux.park(fit->aux_base, fit->aux_bytes)) (void)fit->aux_base.release();
  delete fit;
}

// ---- x = L^-T z for ONE vector ------------------------------------------------------------------------------
// Wide path (n a multiple of 512, n >= 2048): the 512 x 512 diagonal blocks are inverted explicitly (one batched
// triangular solve against the identity), after which a step is two column-dot launches per 512 rows instead of
// four fused launches per 128 rows: the chain is launch-latency-bound.  The width is fixed; no environment switch
// changes it.  Otherwise the 128-row chain on 128 x 128 inverses.  ws: backsolve_ws_elems(n) doubles of scratch.
long long backsolve_width(long long n) {
  constexpr long long BW = 512;
  static_assert(BW <= TALL_MATVEC_MAX_COLS, "forward_solve_vec_wide's launch_tall_matvec takes BW columns");
  return (n >= 4 * BW && n % BW == 0) ? BW : 0;
}

size_t backsolve_ws_elems(long long n) {
  const long long BW = backsolve_width(n);
  const size_t blocks = BW ? (size_t)(n / BW) * (size_t)BW * (size_t)BW : (size_t)((n + NB - 1) / NB) * NB * NB;
  return (size_t)round_up(n, 2) + blocks;
}

// first_done / ev_done: the inverses of the first `first_done` blocks are already being computed on another stream
// (factor_lower's early inversion); ev_done completes when they are there.
void backward_solve_vec_any(hipStream_t s, const double *A, long long n, long long lda, const double *invd,
                            double *z, double *ws, long long first_done, hipEvent_t ev_done) {
  double *xs = ws, *W = ws + round_up(n, 2);
  const long long BW = backsolve_width(n);
  if (!BW) {
    invert_diag_blocks(s, A, n, lda, invd, W);
    backward_solve_vec(s, A, n, lda, W, z, xs);
    return;
  }
  const long long nb = n / BW;
  if (first_done < 0 || first_done > nb) first_done = 0;
  // (first_done == nb - 1 - every inverse but the last block's under way - is backward_solve_vec_from's fast path below)
  if (first_done < nb) {
    const long long cnt = nb - first_done;
    launch_set_identity_batched(s, W + first_done * BW * BW, BW, BW * BW, BW, cnt);
    forward_solve_mat_batched(s, A + first_done * BW * (lda + 1), BW * (lda + 1), BW, lda,
                              invd + first_done * (BW / NB) * (long long)(36 * MB * MB), (BW / NB) * (long long)(36 * MB * MB),
                              W + first_done * BW * BW, BW * BW, BW, BW, /*rhs_lower=*/true, cnt);
  }
  if (first_done > 0 && ev_done) (void)hipStreamWaitEvent(s, ev_done, 0);
  for (long long b = nb - 1; b >= 0; --b) {
    const long long k0 = b * BW;
    launch_colvec_dot(s, W + b * BW * BW, BW, BW, BW, z + k0, 1.0, 0.0, nullptr, xs + k0);  // x_B = inv(L_BB)^T z_B
    if (k0 > 0) launch_colvec_dot(s, A + k0, lda, BW, k0, xs + k0, -1.0, 1.0, z, z);         // z[0:k0] -= L[B, 0:k0]^T x_B
  }
  (void)hipMemcpyAsync(z, xs, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s);
}

// ---- one right-hand side through explicitly inverted BW x BW diagonal blocks (n a multiple of BW): invert_wide_blocks
// (solve.hip) ----------------
// z <- L^-1 z, right-looking: x_B = W_B z_B (in place), z[below] -= L[below, B] x_B: two mat-vec launches per BW rows
// instead of one fused launch per 128 (the chain is launch-latency-bound).  partial: n doubles of scratch.
// A32 (optional): an fp32 copy of the factor's lower triangle (same leading dimension) for the products with the rows
// below / the columns left of a diagonal block - half the bytes of sweeps that are bound by them; for a PRECONDITIONER
void forward_solve_vec_wide(hipStream_t s, const double *A, long long n, long long lda, const double *W, long long BW,
                            double *z, double *partial, const float *A32) {
  const long long nb = n / BW;
  // (BW <= TALL_MATVEC_MAX_COLS, or the launches below do nothing: backsolve_width's static_assert and
  // mixed_precondition_setup check it where the width is chosen)
  for (long long b = 0; b < nb; ++b) {
    const long long k0 = b * BW, below = n - k0 - BW;
    // (x_B goes through `partial` first: the kernel may not overwrite z_B while other workgroups still read it)
    launch_tall_matvec(s, W + b * BW * BW, BW, BW, BW, z + k0, 1.0, 0.0, nullptr, partial);
    (void)hipMemcpyAsync(z + k0, partial, sizeof(double) * (size_t)BW, hipMemcpyDeviceToDevice, s);
    if (below > 0 && A32) launch_tall_matvec_f32(s, A32 + k0 * lda + k0 + BW, lda, below, BW, z + k0, -1.0, 1.0, z + k0 + BW, z + k0 + BW);
    else if (below > 0) launch_tall_matvec(s, A + k0 * lda + k0 + BW, lda, below, BW, z + k0, -1.0, 1.0, z + k0 + BW, z + k0 + BW);
  }
}

// x = L^-T z_in OUT of place (the fit: z = L^-1 y stays, the information vector is written where it lives).  With the
// early inversion under way this is the loop above without its two copy launches: the first update reads z_in and
// writes the work vector (ws[0:n]), every x_B goes straight into x.
void backward_solve_vec_from(hipStream_t s, const double *A, long long n, long long lda, const double *invd, const double *z_in,
                             double *x, double *ws, long long first_done, hipEvent_t ev_done, int *flags) {
  const long long BW = backsolve_width(n), nb = BW ? n / BW : 0;
  // (flags == nullptr: the one-launch substitution of the last block is off - AGP_BACKSUB_COOP=0, or a hand-over timed out
  // earlier on this context)
  if (BW && nb >= 2 && first_done == nb - 1 && flags) {
    double *work = ws, *W = ws + round_up(n, 2);
    const long long k0 = (nb - 1) * BW;
    launch_fill_sentinel(s, x + k0, BW);
    backward_solve_coop(s, A + k0 * (lda + 1), BW, lda, invd + (k0 / NB) * (long long)(36 * MB * MB), z_in + k0, x + k0, flags, nullptr);
    launch_colvec_dot(s, A + k0, lda, BW, k0, x + k0, -1.0, 1.0, z_in, work);  // work[0:k0] = z[0:k0] - L[B, 0:k0]^T x_B
    if (ev_done) (void)hipStreamWaitEvent(s, ev_done, 0);
    for (long long b = nb - 2; b >= 0; --b) {
      const long long c0 = b * BW;
      launch_colvec_dot(s, W + b * BW * BW, BW, BW, BW, work + c0, 1.0, 0.0, nullptr, x + c0);
      if (c0 > 0) launch_colvec_dot(s, A + c0, lda, BW, c0, x + c0, -1.0, 1.0, work, work);
    }
    return;
  }
  (void)hipMemcpyAsync(x, z_in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s);
  backward_solve_vec_any(s, A, n, lda, invd, x, ws, first_done, ev_done);
}

// z <- L^-T z with the same inverses (the loop of backward_solve_vec_any); xs: n doubles of scratch
void backward_solve_vec_wide(hipStream_t s, const double *A, long long n, long long lda, const double *W, long long BW,
                             double *z, double *xs, const float *A32) {
  const long long nb = n / BW;
  for (long long b = nb - 1; b >= 0; --b) {
    const long long k0 = b * BW;
    launch_colvec_dot(s, W + b * BW * BW, BW, BW, BW, z + k0, 1.0, 0.0, nullptr, xs + k0);
    if (k0 > 0 && A32) launch_colvec_dot_f32(s, A32 + k0, lda, BW, k0, xs + k0, -1.0, 1.0, z, z);
    else if (k0 > 0) launch_colvec_dot(s, A + k0, lda, BW, k0, xs + k0, -1.0, 1.0, z, z);
  }
  (void)hipMemcpyAsync(z, xs, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s);
}

// ---- the preconditioner of the mixed fit's refinement (api_internal.h: MixedPreconditioner) ---------------------------
int mixed_precondition_setup(hipStream_t s, const MixedPreconditioner &pc, const double *invd) {
  // (the widths the sweeps' kernels are written for; launch_tall_matvec* would do NOTHING beyond TALL_MATVEC_MAX_COLS and
  // leave the vector of the step before in place)
  if ((pc.BW != 512 && pc.BW != 1024) || pc.BW > TALL_MATVEC_MAX_COLS || pc.n <= 0 || pc.n % pc.BW != 0) return AGP_ERR_INVALID_ARGUMENT;
  invert_wide_blocks(s, pc.A, pc.n, pc.lda, invd, pc.BW, pc.W);
  // ... and their transposes: the forward sweep applies inv(L_BB) as a column-wise product with the transposed copy
  // (one workgroup per output, like the backward sweep) instead of a row-wise one on BW / 64 workgroups
  launch_transpose_blocks(s, pc.W, pc.WT, pc.BW, pc.n / pc.BW);
  if (pc.L32) launch_convert_lower_f32(s, pc.A, pc.lda, pc.n, pc.L32);
  return AGP_OK;
}

// both sweeps out of place - no staging copy per block, none at the end: t1 = in is consumed by the forward sweep
// (x_B into t2, the rows below updated in t1), t2 by the backward sweep (x_B into outv, the rows above updated in t2)
void mixed_precondition_forward(hipStream_t s, const MixedPreconditioner &pc, const double *in) {
  const long long n = pc.n, lda = pc.lda, BW = pc.BW, nbw = n / BW;
  double *t1 = pc.t1, *t2 = pc.t2;
  (void)hipMemcpyAsync(t1, in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s);
  for (long long b = 0; b < nbw; ++b) {
    const long long k0 = b * BW, below = n - k0 - BW;
    launch_colvec_dot(s, pc.WT + b * BW * BW, BW, BW, BW, t1 + k0, 1.0, 0.0, nullptr, t2 + k0);  // x_B = inv(L_BB) z_B
    // (BW <= TALL_MATVEC_MAX_COLS: mixed_precondition_setup)
    if (below > 0) launch_tall_matvec_f32(s, pc.L32 + k0 * lda + k0 + BW, lda, below, BW, t2 + k0, -1.0, 1.0, t1 + k0 + BW, t1 + k0 + BW);
  }
}

void mixed_precondition_backward(hipStream_t s, const MixedPreconditioner &pc, double *outv) {
  const long long n = pc.n, lda = pc.lda, BW = pc.BW, nbw = n / BW;
  double *t2 = pc.t2;
  for (long long b = nbw - 1; b >= 0; --b) {
    const long long k0 = b * BW;
    launch_colvec_dot(s, pc.W + b * BW * BW, BW, BW, BW, t2 + k0, 1.0, 0.0, nullptr, outv + k0);  // x_B = inv(L_BB)^T z_B
    if (k0 > 0) launch_colvec_dot_f32(s, pc.L32 + k0, lda, BW, k0, outv + k0, -1.0, 1.0, t2, t2);
  }
}

void mixed_precondition_apply(hipStream_t s, const MixedPreconditioner &pc, const double *in, double *outv) {
  const long long n = pc.n, lda = pc.lda, BW = pc.BW;
  if (pc.L32) {
    mixed_precondition_forward(s, pc, in);
    mixed_precondition_backward(s, pc, outv);
    return;
  }
  // (no fp32 copy - its allocation failed: the fp64 factor, in place)
  (void)hipMemcpyAsync(outv, in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s);
  forward_solve_vec_wide(s, pc.A, n, lda, pc.W, BW, outv, pc.scratch, nullptr);
  backward_solve_vec_wide(s, pc.A, n, lda, pc.W, BW, outv, pc.scratch, nullptr);
}

namespace {
struct MixedRequest {
  int max_iterations = 0;
  double tolerance = 0.;
  int iterations = 0;       // out
  double residual = 0.;     // out: ||y - K a||_2 / ||y||_2 of the returned information vector
};
}  // namespace

static int refine_information(agp_context_impl *ctx, agp_fit *fit, const double *Kfull, const double *Wfwd,
                              double *vec, MixedRequest *mixed);

static int fit_create_impl(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y,
                           const double *y_var, agp_fit **out, double *information, double *log_det,
                           MixedRequest *mixed) {
  if (!c || !k || !x || !y || !out) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  *out = nullptr;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;

  agp_fit *fit = new (std::nothrow) agp_fit();
  if (!fit) return AGP_ERR_INVALID_ARGUMENT;
  fit->device = ctx->device;
  fit->n = n;
  fit->lda = factor_ld(n);
  const long long nblk = (n + NB - 1) / NB;
  hipStream_t s = ctx->stream;
  fit->ctx = ctx;
  // an early return destroys the fit (its blocks go to the context's slots), the exact covariance of a mixed fit goes back
  // to its slot (parked for the next mixed fit of the same size, like the factor's own buffer), the rest is freed
  FitGuard guard(fit);
  struct ParkK {
    ParkSlot &slot;
    DevMem<double> mem;
    size_t bytes = 0;
    void drop() {
      if (mem && slot.park(mem, bytes)) (void)mem.release();
      mem.reset();
    }
    ~ParkK() { drop(); }
  } Kfull{ctx->pool_K};
  DevMem<double> yvar_d;
  DevMem<double> Wfwd, vec;  // mixed precision only
  fit->A_bytes = sizeof(double) * (size_t)fit->lda * (size_t)n;
  fit->own_A.adopt(static_cast<double *>(ctx->pool_A.take(fit->A_bytes)));
  if (!fit->own_A) AGP_HIP_CHECK(ctx, fit->own_A.alloc_plain(fit->A_bytes));
  fit->A = fit->own_A;
  {
    const size_t n_invd = (size_t)nblk * (36 * MB * MB), n_winv = (size_t)nblk * NB * NB, n_vec = (size_t)round_up(n, 2);
    // (+ train_features = features, un-wrapped; gp.hpp:63,293: always a copy, inside this pooled block - a hipMalloc and a
    // hipFree per fit are ~0.1 ms of a 2 ms fit)
    const size_t n_feat = (size_t)n * ((size_t)x->dim + (x->eq_id ? 1 : 0) + (size_t)x->n_scale_columns);
    fit->aux_bytes = sizeof(double) * (n_invd + n_winv + 2 * n_vec + n_feat);
    fit->aux_base.adopt(static_cast<double *>(ctx->pool_aux.take(fit->aux_bytes)));
    if (!fit->aux_base) AGP_HIP_CHECK(ctx, fit->aux_base.alloc_plain(fit->aux_bytes));
    fit->invd = fit->aux_base;
    fit->winv = fit->invd + n_invd;
    fit->alpha = fit->winv + n_winv;
    fit->z = fit->alpha + n_vec;
  }
  const hipMemcpyKind kind = x->location == AGP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  // device-resident inputs: the copies of the training features and targets travel in the ONE preparation launch of
  // build_and_factor (pub.h: PrepArgs) instead of a copy kernel each; host inputs are uploads and stay what they were
  PrepArgs pre;
  const bool dev_in = x->location != AGP_HOST;
  auto stage = [&](void *dst, const void *src, long long words) -> hipError_t {
    if (dev_in) { pre.copy(dst, src, words); return hipSuccess; }
    return hipMemcpyAsync(dst, src, sizeof(double) * (size_t)words, kind, s);
  };
  {
    double *fcur = fit->z + round_up(n, 2);
    FeatView v;
    v.n = n; v.dim = x->dim; v.nsc = x->n_scale_columns; v.meas = 0;
    v.coords = fcur; v.ids = nullptr; v.scales = nullptr;
    AGP_HIP_CHECK(ctx, stage(fcur, x->coords, n * (long long)x->dim));
    fcur += (size_t)n * (size_t)x->dim;
    if (x->eq_id) {
      v.ids = reinterpret_cast<const long long *>(fcur);
      AGP_HIP_CHECK(ctx, stage(fcur, x->eq_id, n));
      fcur += n;
    }
    if (x->n_scale_columns > 0) {
      v.scales = fcur;
      AGP_HIP_CHECK(ctx, stage(fcur, x->scales, n * (long long)x->n_scale_columns));
    }
    fit->train.v = v;  // (a view into aux_base: DeviceFeatures::release has nothing to free)
  }
  AGP_HIP_CHECK(ctx, stage(fit->z, y, n));
  if (y_var) {
    AGP_HIP_CHECK(ctx, yvar_d.alloc_plain(sizeof(double) * (size_t)n));
    AGP_HIP_CHECK(ctx, stage(yvar_d, y_var, n));
  }
  if (x->location == AGP_HOST) AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  if (mixed && pre.n > 0) {  // (the mixed fit reads the staged inputs before build_and_factor: its exact covariance, the copy of y)
    launch_prep(s, pre);
    pre = PrepArgs();
  }
  FeatView xm = fit->train.v;
  xm.meas = 1;  // as_measurements(features), gp.hpp:288
  // what this fit asks of its factorisation: the low-precision bulk update of the mixed fit, the early inversion of the
  // wide diagonal blocks of the deferred fp64 fit - and what the factorisation reports back
  FactorRequest req;
  FactorOutcome factored;
  if (mixed) {
    // the exact fp64 covariance (lower triangle: the refinement multiplies with launch_symv_lower) for the residuals, the targets,
    // and the work vectors r, z, p, q
    Kfull.bytes = fit->A_bytes;
    Kfull.mem.adopt(static_cast<double *>(ctx->pool_K.take(Kfull.bytes)));
    if (!Kfull.mem) {
      ctx->pool_K.clear();  // (a block of another size goes BEFORE this one is allocated: both are of the factor's size)
      AGP_HIP_CHECK(ctx, Kfull.mem.alloc_plain(Kfull.bytes));
    }
    AGP_HIP_CHECK(ctx, Wfwd.alloc_plain(sizeof(double) * (size_t)nblk * NB * NB));
    AGP_HIP_CHECK(ctx, vec.alloc_plain(sizeof(double) * (size_t)n * 5));
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(vec, fit->z, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    launch_gram(s, dprog, xm, xm, /*symmetric=*/true, /*lower_only=*/true, Kfull.mem, fit->lda, yvar_d, ctx->d_flags,
                &k->prog);
    // fp32-accurate products of the bulk updates: on the 16-bit matrix pipe from split planes of the panel - default
    // (round 6): two fp16 planes of power-of-two-scaled rows; AGP_MIXED_F16=0: three bf16 planes - or - AGP_MIXED_BF16=0 -
    // on the fp32 MFMA as in rounds 1-4
    req.products = !ctx->tune.mixed_bf16 ? BulkProducts::Fp32 : (ctx->tune.mixed_f16 ? BulkProducts::F16x2 : BulkProducts::Bf16x3);
    req.nbo_wide = (uses_planes(req.products) && ctx->tune.mixed_nbo > 512 && ctx->tune.mixed_nbo % 128 == 0) ? ctx->tune.mixed_nbo : 0;
    PanelStager::reserve(ctx, req.products, n, req.nbo_wide);
  }
  // The fp64 fit does not wait for the factorisation before it enqueues the backward substitution: one host round trip
  // (~0.1 ms) less; the status is read after the single synchronisation at the end, and a substitution through a factor
  // that turns out not to be positive definite was wasted work on garbage, nothing more.  (The flags and the
  // log-determinant are copied to the host right behind the factorisation, before the substitution touches d_scalars.)
  const bool deferred = !mixed && !yvar_d;
  // information = L^-T z in ONE launch (solve.hip: backsub_coop_kernel) for the fp64 fit: its output vector is the
  // hand-over buffer and is sentinel-filled by the preparation launch.  (The refinement of a mixed fit needs the
  // inverted diagonal blocks anyway and keeps the launch-per-block substitution.)
  // Measured (profiles/r05): one hand-over + substitution per 128-column block is ~9 us - 37 us at N = 512 against 45 us
  // for the launch chain, 286 us at N = 4096 against 190 us through the 512-wide inverted blocks: small fits only.
  const bool coop = !mixed && ctx->tune.backsub_coop && n <= ctx->tune.backsub_coop_max;
  // (hand-over: the sentinel-filled output itself up to BACKSUB_DIRECT_BLOCKS blocks, per-block flags in the unused
  // block-inverse buffer beyond)
  const bool coop_direct = coop && (n + NB - 1) / NB <= BACKSUB_DIRECT_BLOCKS;
  ctx->sched.reset_factor(n);
  ctx->sched.backsub = coop ? (coop_direct ? ctx->sched.BS_COOP_DIRECT : ctx->sched.BS_COOP_FLAGS)
                            : (backsolve_width(n) ? ctx->sched.BS_WIDE : ctx->sched.BS_CHAIN);
  ctx->sched.bs_done = 0;
  if (coop && coop_direct) pre.sentinel(fit->alpha, n);
  else if (coop) pre.fill(fit->winv, 0ull, backsub_done_words(n, 1));
  FactorTimers ftimers;
  if (!coop && deferred && backsolve_width(n)) {
    // the inverses of the wide diagonal blocks for the backward substitution: computed by factor_lower on its idle
    // second stream while the chain-bound tail of the factorisation runs (factor_plan.h: FactorRequest)
    if (reserve_ws(ctx, ctx->ws_aux, sizeof(double) * backsolve_ws_elems(n)) == AGP_OK) {
      req.inv_W = ctx->ws_aux + round_up(n, 2);
      req.inv_BW = backsolve_width(n);
    }
  }
  // (a deferred fit with the one-launch substitution: that launch's last workgroup writes the status block into the
  // pinned mirror - no copy launch behind the factorisation, none behind the substitution)
  const bool status_in_kernel = coop && deferred && ctx->h_status_dev != nullptr;
  st = build_and_factor(ctx, dprog, &k->prog, xm, fit->A, fit->lda, fit->invd, fit->z, yvar_d, !deferred, &ftimers, &pre,
                        !status_in_kernel, mixed ? Kfull.mem.get() : nullptr, req, &factored);
  const long long bs_done = factored.inv_done;
  ctx->sched.bs_done = bs_done;
  yvar_d.reset();  // (here, not at scope exit: the free synchronises the device)
  if (st != AGP_OK) {
    // (the early inversion may still be writing ws_aux on the second stream: whatever uses it next is ordered behind it)
    if (bs_done > 0) (void)hipStreamWaitEvent(s, ctx->ev_inv, 0);
    return st;
  }
  if (!deferred) {
    st = status_from_flags(ctx);
    fit->failed_pivot = ctx->h_flags[1] ? (int64_t)ctx->h_flags[1] - 1 : -1;
    fit->log_det = 2. * ctx->h_scalars[0];
    if (st != AGP_OK) {
      // keep a handle so the caller can query the failed pivot, but no factor
      fit->fail_status = st;
      *out = guard.release();
      return st;
    }
  }
  // information = L^-T (L^-1 y)
  if (ctx->profiling) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[3], s));
  if (coop) {
    TraceRange tr("agp: backward substitution (information = ldlt.solve(y), gp.hpp:68)");
    backward_solve_coop(s, fit->A, n, fit->lda, fit->invd, fit->z, fit->alpha, ctx->d_flags,
                        coop_direct ? nullptr : reinterpret_cast<unsigned long long *>(fit->winv), 1, 0, 0, 0, 0, 0,
                        status_in_kernel ? ctx->d_flags : nullptr, ctx->h_status_dev, (int)(STATUS_BYTES / 8));
    // (the hand-over flag of the substitution: the 48-byte status copy left before it ran)
    if (!status_in_kernel) AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_flags, ctx->d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  } else {
    const int st2 = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * backsolve_ws_elems(n));
    if (st2 != AGP_OK) return st2;
    {
      TraceRange tr("agp: backward substitution (information = ldlt.solve(y), gp.hpp:68)");
      backward_solve_vec_from(s, fit->A, n, fit->lda, fit->invd, fit->z, fit->alpha, ctx->ws_aux, bs_done, ctx->ev_inv,
                              ctx->tune.backsub_coop ? ctx->d_flags : nullptr);
      // (its last wide block goes through the one-launch substitution, which records a timed-out hand-over in flags[2]: the
      // status block left for the host BEFORE the substitution ran - the flags once more behind it)
      if (deferred) AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_flags, ctx->d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    // the refinement steps of the mixed-precision fit use the 128-row chain on fit->winv
    if (mixed) invert_diag_blocks(s, fit->A, n, fit->lda, fit->invd, fit->winv);
  }
  if (mixed) {
    fit->mixed = true;
    invert_diag_blocks_forward(s, n, fit->invd, Wfwd);
    const int st3 = refine_information(ctx, fit, Kfull.mem, Wfwd, vec, mixed);
    Kfull.drop();  // (these three here, not at scope exit: a free synchronises the device)
    Wfwd.reset();
    vec.reset();
    if (st3 != AGP_OK) return st3;
  }
  if (ctx->profiling) AGP_HIP_CHECK(ctx, hipEventRecord(ctx->stage_ev[4], s));
  // (deferred status: the caller's buffer is written only once the factor is known to be good - a NaN, a non-positive
  // pivot or a timed-out hand-over leaves it untouched)
  if (information && !deferred) AGP_HIP_CHECK(ctx, hipMemcpyAsync(information, fit->alpha, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  if (deferred) {
    finish_factor(ctx, ftimers);
    st = status_from_flags(ctx);
    fit->failed_pivot = ctx->h_flags[1] ? (int64_t)ctx->h_flags[1] - 1 : -1;
    fit->log_det = 2. * ctx->h_scalars[0];
    if (st != AGP_OK) {  // keep a handle so the caller can query the failed pivot, but no factor
      fit->fail_status = st;
      *out = guard.release();
      return st;
    }
    if (information) AGP_HIP_CHECK(ctx, hipMemcpy(information, fit->alpha, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  } else if (coop && ctx->h_flags[2]) {  // the one-launch substitution gave up on a hand-over (its producer died)
    ctx->last_error = "back substitution: hand-over timed out";
    return AGP_ERR_HIP;
  }
  if (ctx->profiling) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->stage_ev[3], ctx->stage_ev[4]);
    ctx->stage_ms[2] = ms;
  }
  if (log_det) *log_det = fit->log_det;
  *out = guard.release();
  return AGP_OK;
}

// A hand-over of the step launches that timed out (flags[2]: fewer workgroup slots than the launch layout assumed - a CU
// mask, a partition - so that waiters sat in front of their producers) is not the caller's problem: the fit is repeated
// once on the two-launch schedule, which waits for nothing inside a launch, and the context stays on it.
static int fit_create_retrying(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
                               agp_fit **out, double *information, double *log_det, MixedRequest *mixed) {
  int st = fit_create_impl(c, k, x, y, y_var, out, information, log_det, mixed);
  if (c && c->h_flags) c->sched.handover_timeout = c->h_flags[2];
  if (st == AGP_ERR_HIP && c && c->h_flags && c->h_flags[2] && (c->tune.step_below > 0 || c->tune.panel_fused || c->tune.merge_above > 0)) {
    if (out && *out) { agp_fit_destroy(*out); *out = nullptr; }
    c->tune.step_below = 0;
    c->tune.panel_fused = false;
    c->tune.backsub_coop = false;  // (the one-launch substitution hands over inside a launch too)
    c->tune.merge_above = 0;       // (... and the gate of a merged bulk update waits for another stream's launch)
    ++c->sched.demotions;
    st = fit_create_impl(c, k, x, y, y_var, out, information, log_det, mixed);
    if (c->h_flags) c->sched.handover_timeout = c->h_flags[2];
  }
  return st;
}

int agp_fit_create(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y,
                   const double *y_var, agp_fit **out, double *information, double *log_det) {
  return fit_create_retrying(c, k, x, y, y_var, out, information, log_det, nullptr);
}

int agp_fit_create_mixed(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y,
                         const double *y_var, int max_iterations, double tolerance, agp_fit **out,
                         double *information, double *log_det, int *iterations, double *residual) {
  if (max_iterations < 0 || !(tolerance >= 0.)) return AGP_ERR_INVALID_ARGUMENT;
  MixedRequest m;
  m.max_iterations = max_iterations;
  m.tolerance = tolerance;
  const int st = fit_create_retrying(c, k, x, y, y_var, out, information, log_det, &m);
  if (iterations) *iterations = m.iterations;
  if (residual) *residual = m.residual;
  return st;
}

// Conjugate gradients on K a = y in fp64, preconditioned with the mixed-precision factor (M = L L^T,
// ||I - M^-1 K|| ~ cond(K) * 2^-24): fit->alpha enters as M^-1 y and leaves as K^-1 y to the requested
// relative residual.  vec: 5 n doubles, vec[0:n] = y on entry.
static int refine_information(agp_context_impl *ctx, agp_fit *fit, const double *Kfull, const double *Wfwd,
                              double *vec, MixedRequest *mixed) {
  hipStream_t s = ctx->stream;
  const long long n = fit->n, lda = fit->lda;
  double *yv = vec, *r = vec + n, *z = vec + 2 * n, *p = vec + 3 * n, *q = vec + 4 * n;
  double *xa = fit->alpha;
  double *dots = ctx->d_scalars;  // 4 device doubles (log-det already read back)
  auto read_dots = [&](int count, double *host) -> int {
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_scalars, dots, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, s));
    AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
    for (int i = 0; i < count; ++i) host[i] = ctx->h_scalars[i];
    return AGP_OK;
  };
  // the substitutions of every step: through 512-wide inverted diagonal blocks when the size allows (2 x n / 512
  // mat-vec launches per direction instead of n / 128 fused steps: the chains are launch-latency-bound)
  // (1024-wide inverted blocks here: the eight-odd preconditioner applications share one inversion, and half as many
  // launch-bound block steps per sweep are worth 5 ms at N = 32768; a single substitution is better off with 512)
  long long BW = backsolve_width(n);
  if (BW == 512 && n % 1024 == 0 && n >= 8192) BW = 1024;
  // the mat-vec's workspace and the inverted blocks (268 MB at N = 32768): kept in the context between mixed fits - a
  // hipMalloc + hipFree pair of that size per fit was 2-3 ms of a 120 ms fit
  const size_t symv_elems = (symv_ws_elems(n) + 1) / 2 * 2;
  const size_t wide_elems = BW ? (size_t)(n / BW) * (size_t)BW * (size_t)BW : 0;
  const size_t np2 = (size_t)round_up(n, 2);
  {
    const int st_ws = reserve_ws(ctx, ctx->ws_refine, sizeof(double) * (symv_elems + 2 * wide_elems + 2 * np2));
    if (st_ws != AGP_OK) return st_ws;
  }
  double *symv_ws = ctx->ws_refine;
  double *Wwide = BW ? ctx->ws_refine + symv_elems : nullptr;
  double *WwideT = BW ? Wwide + wide_elems : nullptr;
  double *t1 = ctx->ws_refine + symv_elems + 2 * wide_elems, *t2 = t1 + np2;  // the sweeps' work vectors
  // The preconditioner M = L L^T is applied eight-odd times and each application streams L twice; it does not have to
  // be exact - L itself comes from fp32-rounded products -, so the sweeps read an fp32 COPY of L's off-diagonal blocks
  // (the inverted diagonal blocks stay fp64): half the bytes, kept in the context between fits.
  float *L32 = nullptr;
  if (BW) {
    const size_t want = sizeof(float) * (size_t)lda * (size_t)n;
    // (the slot's occupant when it has this size, else a new block in its place; it stays in the slot while it is used)
    L32 = static_cast<float *>(ctx->pool_L32.take(want));
    if (!L32) {
      ctx->pool_L32.clear();
      if (dev_malloc_plain_bytes(reinterpret_cast<void **>(&L32), want) != 0) { (void)hipGetLastError(); L32 = nullptr; }
    }
    if (L32) (void)ctx->pool_L32.park(L32, want);
  }
  MixedPreconditioner pc;
  pc.A = fit->A; pc.n = n; pc.lda = lda; pc.BW = BW;
  pc.W = Wwide; pc.WT = WwideT; pc.L32 = L32;
  pc.t1 = t1; pc.t2 = t2; pc.scratch = ctx->ws_aux;
  if (BW) {
    const int st_pc = mixed_precondition_setup(s, pc, fit->invd);
    if (st_pc != AGP_OK) return st_pc;
  }
  auto precondition = [&](const double *in, double *outv) {
    if (BW) {
      mixed_precondition_apply(s, pc, in, outv);
    } else {
      (void)hipMemcpyAsync(outv, in, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s);
      forward_solve_vec(s, fit->A, n, lda, Wfwd, outv, ctx->ws_aux);
      backward_solve_vec(s, fit->A, n, lda, fit->winv, outv, ctx->ws_aux);
    }
  };
  double h[4];
  int st;
  // r = y - K a
  launch_symv_lower(s, Kfull, lda, n, xa, -1., 1., yv, r, symv_ws);
  launch_dot(s, yv, yv, n, dots + 0);
  launch_dot(s, r, r, n, dots + 1);
  if ((st = read_dots(2, h)) != AGP_OK) return st;
  const double ynorm = std::sqrt(h[0]);
  double rnorm = std::sqrt(h[1]);
  const double target = mixed->tolerance * ynorm;
  int it = 0;
  if (rnorm > target && mixed->max_iterations > 0) {
    precondition(r, z);
    (void)hipMemcpyAsync(p, z, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s);
    launch_dot(s, r, z, n, dots + 0);
    if ((st = read_dots(1, h)) != AGP_OK) return st;
    double rz = h[0];
    double best = rnorm;
    int stalled = 0;
    while (it < mixed->max_iterations && rnorm > target) {
      launch_symv_lower(s, Kfull, lda, n, p, 1., 0., nullptr, q, symv_ws);
      launch_dot(s, p, q, n, dots + 0);
      if ((st = read_dots(1, h)) != AGP_OK) return st;
      if (!(h[0] > 0.) || !(rz > 0.)) break;  // breakdown: K or the preconditioner lost definiteness
      const double a = rz / h[0];
      launch_axpby(s, n, a, p, 1., xa, xa);
      launch_axpby(s, n, -a, q, 1., r, r);
      ++it;
      precondition(r, z);
      launch_dot(s, r, r, n, dots + 0);
      launch_dot(s, r, z, n, dots + 1);
      if ((st = read_dots(2, h)) != AGP_OK) return st;
      rnorm = std::sqrt(h[0]);
      if (rnorm < 0.9 * best) { best = rnorm; stalled = 0; }
      else if (++stalled >= 3) break;  // at the fp64 floor of this system
      const double beta = h[1] / rz;
      rz = h[1];
      launch_axpby(s, n, 1., z, beta, p, p);
    }
    // report the TRUE residual of what is returned (the recurrence drifts)
    launch_symv_lower(s, Kfull, lda, n, xa, -1., 1., yv, r, symv_ws);
    launch_dot(s, r, r, n, dots + 0);
    if ((st = read_dots(1, h)) != AGP_OK) return st;
    rnorm = std::sqrt(h[0]);
  }
  mixed->iterations = it;
  mixed->residual = ynorm > 0. ? rnorm / ynorm : rnorm;
  return AGP_OK;
}

int64_t agp_fit_size(const agp_fit *fit) { return fit ? fit_real_rows(fit) : 0; }
int64_t agp_fit_failed_pivot(const agp_fit *fit) { return fit ? fit->failed_pivot : -1; }

int agp_fit_log_determinant(const agp_fit *fit, double *out) {
  if (!fit || !out) return AGP_ERR_INVALID_ARGUMENT;
  *out = fit->log_det;
  return AGP_OK;
}

int agp_fit_download_information(agp_context *ctx, const agp_fit *fit, double *information) {
  if (!ctx || !fit || !information || !fit->alpha) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!fit->phantom.empty()) return fit_compact_vector(ctx, fit, fit->alpha, information, AGP_HOST);
  return copy_out(ctx, fit->alpha, fit->n, information, AGP_HOST);
}

int agp_fit_download_factor(agp_context *ctx, const agp_fit *fit, double *L, int64_t ld) {
  if (!ctx || !fit || !L || ld < fit_real_rows(fit)) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const long long n = fit->n;
  if (!fit->phantom.empty()) {
    // drop the phantom rows AND columns: they are decoupled (identity rows), what remains is the factor of the real matrix
    const long long nr = fit_real_rows(fit), ldt = round_up(nr, 2);
    int st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * ((size_t)fit->lda * (size_t)n + (size_t)ldt * (size_t)n));
    if (st != AGP_OK) return st;
    double *full = ctx->ws_aux, *rows = full + (size_t)fit->lda * (size_t)n;
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(full, fit->A, sizeof(double) * (size_t)fit->lda * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    launch_zero_upper(ctx->stream, full, fit->lda, n);
    if ((st = fit_compact_matrix(ctx, fit, full, fit->lda, n, rows, ldt, AGP_DEVICE)) != AGP_OK) return st;  // rows: nr x n
    // columns: one strided copy per run of real columns
    long long pad = 0, real = 0;
    auto copy_cols = [&](long long p0, long long r0, long long len) -> int {
      return copy_out_2d(ctx, rows + p0 * ldt, ldt, nr, len, L + r0 * ld, ld, AGP_HOST);
    };
    for (const auto &ph : fit->phantom) {
      if (ph.first > pad) { if ((st = copy_cols(pad, real, ph.first - pad)) != AGP_OK) return st; real += ph.first - pad; }
      pad = ph.second;
    }
    if (n > pad && (st = copy_cols(pad, real, n - pad)) != AGP_OK) return st;
    return AGP_OK;
  }
  int st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (size_t)fit->lda * (size_t)n);
  if (st != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->ws_aux, fit->A, sizeof(double) * (size_t)fit->lda * (size_t)n,
                                    hipMemcpyDeviceToDevice, ctx->stream));
  launch_zero_upper(ctx->stream, ctx->ws_aux, fit->lda, n);
  return copy_out_2d(ctx, ctx->ws_aux, fit->lda, n, n, L, ld, AGP_HOST);
}

// ---- nll -------------------------------------------------------------------
int agp_nll(agp_context *c, const agp_kernel *k, const agp_features *x, const double *y, const double *y_var,
            double *out) {
  if (!c || !k || !x || !y || !out) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(x);
  if (st != AGP_OK) return st;
  const long long n = x->n;
  if (n <= 0) return AGP_ERR_INVALID_ARGUMENT;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  const BatchGeometry g = batch_geometry(n, 1);
  const long long lda = g.lda;
  WsLayout size;
  carve_fit(size, g);
  if ((st = reserve_ws(ctx, ctx->ws_A, size.bytes())) != AGP_OK) return st;
  WsLayout ws(ctx->ws_A);
  const FitRegions r = carve_fit(ws, g);
  double *A = r.A, *invd = r.invd, *z = r.z, *yvar_d = y_var ? r.yvar : nullptr;
  DeviceFeatures dx;
  if ((st = to_device(ctx, x, false, &dx)) != AGP_OK) return st;
  if ((st = vector_to_device(ctx, y, n, x->location, z)) != AGP_OK) { dx.release(); return st; }
  if (y_var && (st = vector_to_device(ctx, y_var, n, x->location, yvar_d)) != AGP_OK) { dx.release(); return st; }
  FeatView xm = dx.v;
  xm.meas = 1;
  st = build_and_factor(ctx, dprog, &k->prog, xm, A, lda, invd, z, yvar_d);
  if (st == AGP_OK) st = status_from_flags(ctx);
  if (st == AGP_OK) {
    // mahalanobis = y^T K^-1 y = z^T z with z = L^-1 y   (likelihood.hpp:44)
    launch_dot(ctx->stream, z, z, n, ctx->d_scalars + 1);
    hipError_t e = hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); st = AGP_ERR_HIP; }
    else {
      const double log_det = 2. * ctx->h_scalars[0];
      *out = 0.5 * (log_det + ctx->h_scalars[1] + (double)n * std::log(2 * M_PI));  // likelihood.hpp:46
    }
  }
  dx.release();
  return st;
}

// `bytes` of the context's pinned staging area (common.h: h_stage), grown on demand; nullptr if it cannot be had (the
// callers then stage through pageable memory and synchronise once).  The previous contents are dead: every user ends its
// call with a synchronisation of the stream that read them.
void *host_stage(agp_context *ctx, size_t bytes) {
  if (ctx->h_stage_bytes < bytes) {
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    ctx->h_stage = nullptr;
    ctx->h_stage_bytes = 0;
    const size_t want = (bytes + 65535) / 65536 * 65536;
    if (hipHostMalloc(&ctx->h_stage, want) != hipSuccess) { (void)hipGetLastError(); ctx->h_stage = nullptr; return nullptr; }
    ctx->h_stage_bytes = want;
  }
  return ctx->h_stage;
}

// ---- tuner objective batching ---------------------------------------------------------
// The negative log likelihoods of `count` parameter vectors of one model on one dataset, in lock step:
// what compute_gradient (tune/finite_difference.hpp:20-94) and the ModelTuner objective
// (tune/tune.hpp:151-161,276-290) evaluate one after the other.  `count` Gram matrices are built into
// slabs and factored by the batched kernels (blockIdx.y = parameter vector), so small and medium N pay
// the launch chain once instead of `count` times.  A parameter vector whose covariance is not positive
// definite (or has NaN) yields NaN in its slot, like the reference's NaN metric (tune.hpp:163-165).
// On the shared front end (batch_front.h): memory from ws_A (batch_layout.h: carve_nll_batch), the context's one status
// block for all problems and no NaN flags from the Gram, one shared variance vector, never the look-ahead schedule.
int agp_nll_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                  const double *y, int64_t ldy, const double *y_var, double *out) {
  if (!c || !y || !out) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  long long n = 0;
  int st = check_batch_problems(count, kernels, features, ldy, nullptr, 0, &n);
  if (st != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const BatchGeometry g = batch_geometry(n, count);
  hipStream_t s = ctx->stream;
  const bool fused_panels = batched_fused_panels(ctx, g, /*allow_lookahead=*/false);
  const size_t table_bytes = gram_batch_table_bytes(count);
  WsLayout size;
  carve_nll_batch(size, g, fused_panels, table_bytes);
  if ((st = reserve_ws(ctx, ctx->ws_A, size.bytes())) != AGP_OK) return st;
  WsLayout ws(ctx->ws_A);
  const NllBatchRegions r = carve_nll_batch(ws, g, fused_panels, table_bytes);
  const int loc = features[0]->location;
  if ((st = upload_problem_columns(ctx, y, ldy, n, count, loc, r.ys, g.np2)) != AGP_OK) return st;
  if (y_var && (st = upload_problem_columns(ctx, y_var, n, n, 1, loc, r.yvar, g.np2)) != AGP_OK) return st;
  if (loc == AGP_HOST) AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  {  // one preparation launch: log sums and flags zeroed, the hand-over buffers of the fused panel launches sentinel-filled
    PrepArgs prep;
    prep.fill(r.logsum, 0ull, g.cp2);
    prep.fill(ctx->d_flags, 0ull, 2);
    launch_batch_prep(s, prep, g, r.invd, r.zpub);
  }
  BatchGramTables tables(g, kernels, r.A, y_var ? r.yvar : nullptr, 0, nullptr, 0);
  if ((st = tables.upload_features(ctx, features)) != AGP_OK) return st;
  if ((st = launch_batch_grams(ctx, g, tables, kernels, r.gram_table, count > 1 ? host_stage(ctx, table_bytes) : nullptr)) != AGP_OK)
    return st;
  factor_batch(ctx, g, /*allow_lookahead=*/false, r.A, r.invd, r.ys, ctx->d_flags, 0, r.logsum, r.zpub);
  launch_coldot(s, r.ys, g.np2, r.ys, g.np2, n, count, r.quad, -1.0, nullptr);  // z_b^T z_b, z_b = L_b^-1 y_b
  std::vector<double> h(2 * (size_t)g.cp2);  // [logsum | quad]
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), r.logsum, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  for (int b = 0; b < count; ++b)  // likelihood.hpp:38-47
    out[b] = 0.5 * (2. * h[(size_t)b] + h[(size_t)g.cp2 + (size_t)b] + (double)n * std::log(2 * M_PI));
  return AGP_OK;
}

// problem's training features inside the slab of its batch: coordinates, equality ids, scale columns, each of the n rows
// of the batch (a ragged problem has fewer of its own: the rest are phantom rows)
static FeatView carve_features(WsLayout &ws, const agp_features *f, long long n) {
  FeatView v;
  v.n = n; v.dim = f->dim; v.nsc = f->n_scale_columns; v.meas = 0;
  v.coords = ws.take<double>((size_t)n * (size_t)f->dim);
  v.ids = f->eq_id ? ws.take<long long>((size_t)n) : nullptr;
  v.scales = f->n_scale_columns > 0 ? ws.take<double>((size_t)n * (size_t)f->n_scale_columns) : nullptr;
  return v;
}

}  // extern "C"

// B independent fits of one shape in lock step: the Fit<GPFit> constructor (models/gp.hpp:61-69) for `count` datasets /
// parameter vectors at once.  Where the reference's users live - N of a few hundred to a few thousand
// (benchmarks/bench_predict.cc:20-40, the tuner loop tune/tune.hpp:276-290) - ONE fit is bound by the latency of its
// 128 serial pivots per panel (27-30 us per POTRF, config 2: 0.14 of the MFMA peak); a batch shares that latency and
// fills the chip with the trailing updates of all problems (factor_lower_batched).
// On the shared front end (batch_front.h): one allocation of its own that the fits keep (batch_layout.h:
// carve_fit_batch, then each problem's training features), the tables of the call from dev_malloc
// (carve_fit_batch_tables), status words per problem, the look-ahead schedule where the predicate asks for it.
//
// `ragged` (agp_fit_create_batch_ragged) admits problems of unequal sizes n_b.  The padded size n of the call is the
// largest of them; problem b is the fit of diag(K_b, I) with the trailing phantom rows [n_b, n) (common.h:
// agp_fit::phantom).  Its Gram launch runs on a view of the n_b real rows - so the NaN flag and the target variances are
// those of real rows only -, one table-driven pad launch behind it writes the phantom rows of the slab, of z and of the
// training features (ragged_batch.hip), and from there on the chain below is the one of equal sizes at size n.  With all
// sizes equal nothing is padded and the two entries run the same launches.  A ragged call checks every argument before
// it writes anything, out and status included.
int agp::fit_create_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                          const double *y, int64_t ldy, const double *y_var, int64_t ldv, agp_fit **out, double *information,
                          int64_t ldi, double *log_det, int *status, bool ragged) {
  if (!c || count <= 0 || count > BATCH_MAX_PROBLEMS || !kernels || !features || !y || !out || !status) return AGP_ERR_INVALID_ARGUMENT;
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  long long n = 0;
  bool equal = true;
  int st = AGP_OK;
  if (ragged) {
    if ((st = check_batch_problems_ragged(count, kernels, features, ldy, y_var, ldv, &n, &equal)) != AGP_OK) return st;
    if (information && ldi < n) return AGP_ERR_INVALID_ARGUMENT;
  }
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  for (int b = 0; b < count; ++b) { out[b] = nullptr; status[b] = AGP_ERR_INVALID_ARGUMENT; }
  if (!ragged) {
    if ((st = check_batch_problems(count, kernels, features, ldy, y_var, ldv, &n)) != AGP_OK) return st;
    if (information && ldi < n) return AGP_ERR_INVALID_ARGUMENT;
  }
  const bool padded = !equal;  // some problem has phantom rows
  const BatchGeometry g = batch_geometry(n, count);
  hipStream_t s = ctx->stream;
  WsLayout size;
  carve_fit_batch(size, g, y_var != nullptr);
  for (int b = 0; b < count; ++b) carve_features(size, features[b], n);
  const size_t bytes = size.bytes();
  DevMem<double> base;
  base.adopt(static_cast<double *>(ctx->pool_batch.take(bytes)));
  if (!base) {
    ctx->pool_batch.clear();  // (a slab of another size goes BEFORE this one is allocated)
    AGP_HIP_CHECK(ctx, base.alloc_plain(bytes));
  }
  WsLayout ws(base.get());
  const FitBatchRegions r = carve_fit_batch(ws, g, y_var != nullptr);
  std::vector<agp_fit *> fits((size_t)count, nullptr);
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(s);
    for (auto *f : fits)
      if (f) delete f;
    base.reset();
    return code;
  };
#define BATCH_CHECK(expr)                                                     \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess) {                                                   \
      ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);    \
      return fail(AGP_ERR_HIP);                                               \
    }                                                                         \
  } while (0)
  const int loc = features[0]->location;
  const hipMemcpyKind kind = loc == AGP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (!padded) {
    if ((st = upload_problem_columns(ctx, y, ldy, n, count, loc, r.z, g.np2)) != AGP_OK) return fail(st);
    if (y_var && (st = upload_problem_columns(ctx, y_var, ldv, n, count, loc, r.yvar, g.np2)) != AGP_OK) return fail(st);
  }
  // train_features = features (gp.hpp:63): a copy per fit, inside the batch's allocation (no allocation per problem).
  // Device-resident inputs: ONE table-driven copy launch for all problems (pub.h: CopyItem) instead of a copy kernel per array
  std::vector<CopyItem> copies;
  long long copy_max = 0;
  auto stage = [&](const void *dst, const void *src, long long words) -> hipError_t {
    if (!dst) return hipSuccess;  // (an array the problem does not have)
    if (loc == AGP_HOST) return hipMemcpyAsync(const_cast<void *>(dst), src, sizeof(double) * (size_t)words, kind, s);
    copies.push_back(CopyItem{static_cast<unsigned long long *>(const_cast<void *>(dst)), static_cast<const unsigned long long *>(src), words});
    if (words > copy_max) copy_max = words;
    return hipSuccess;
  };
  // (a padded call: the n_b values of column b of the targets and variances go the same way, what follows them in the
  // column is never read; the scale columns land at the stride n of the padded features)
  std::vector<RaggedPadItem> pads(padded ? (size_t)count : 0);
  for (int b = 0; b < count; ++b) {
    agp_fit *fit = new (std::nothrow) agp_fit();
    if (!fit) return fail(AGP_ERR_INVALID_ARGUMENT);
    fits[(size_t)b] = fit;
    const agp_features *f = features[b];
    const long long nb = f->n;
    const FeatView v = carve_features(ws, f, n);
    BATCH_CHECK(stage(v.coords, f->coords, nb * (long long)f->dim));
    BATCH_CHECK(stage(v.ids, f->eq_id, nb));
    if (nb == n) BATCH_CHECK(stage(v.scales, f->scales, n * (long long)f->n_scale_columns));
    else
      for (int k = 0; k < f->n_scale_columns; ++k) BATCH_CHECK(stage(v.scales + (size_t)k * (size_t)n, f->scales + (size_t)k * (size_t)nb, nb));
    fit->train.v = v;  // (not owned: DeviceFeatures::release has nothing to free)
    if (padded) {
      BATCH_CHECK(stage(r.z + (size_t)b * (size_t)g.np2, y + (size_t)b * (size_t)ldy, nb));
      if (y_var) BATCH_CHECK(stage(r.yvar + (size_t)b * (size_t)g.np2, y_var + (size_t)b * (size_t)ldv, nb));
      RaggedPadItem &pi = pads[(size_t)b];
      pi.A = r.A + (size_t)b * (size_t)g.stride_A;
      pi.z = r.z + (size_t)b * (size_t)g.np2;
      pi.coords = const_cast<double *>(v.coords);
      pi.ids = const_cast<long long *>(v.ids);
      pi.scales = const_cast<double *>(v.scales);
      pi.nb = nb;
      pi.dim = f->dim;
      pi.nsc = f->n_scale_columns;
    }
  }
  // device scratch of the call: the copy table and the Gram table of the batched launches, the z slots of the fused panels
  const bool fused_panels = batched_fused_panels(ctx, g, /*allow_lookahead=*/true);
  // (the pad table of a padded call follows the copy table in the same region)
  const size_t copy_items_bytes = sizeof(CopyItem) * copies.size(), pad_bytes = sizeof(RaggedPadItem) * pads.size();
  const size_t pad_off = padded ? (copy_items_bytes + 15) / 16 * 16 : copy_items_bytes;
  const size_t copy_bytes = pad_off + pad_bytes, gram_bytes = gram_batch_table_bytes(count);
  WsLayout tsize;
  carve_fit_batch_tables(tsize, g, fused_panels, copy_bytes, gram_bytes);
  DevMem<void> tables;
  if (tables.alloc_cached(tsize.bytes()) != 0) (void)hipGetLastError();
  WsLayout tws(tables.get());
  const FitBatchTables t = carve_fit_batch_tables(tws, g, fused_panels, copy_bytes, gram_bytes);  // (all null without `tables`)
  // (both tables are built in the context's pinned staging area, laid out like the device's: no synchronisation between
  // the uploads and the launches that read them - the two mid-call synchronisations of round 5 were ~4 % of a batch of
  // 256 fits of N = 512)
  const size_t gram_off = (size_t)(static_cast<char *>(t.gram_table) - static_cast<char *>(t.copy_table));
  char *pinned = tables ? static_cast<char *>(host_stage(ctx, gram_off + gram_bytes)) : nullptr;
  if (padded && !tables) {
    ctx->last_error = "agp_fit_create_batch_ragged: descriptor tables";
    return fail(AGP_ERR_HIP);
  }
  std::vector<char> pageable_tables;
  if (copy_bytes > 0) {
    if (tables) {
      char *src = pinned;
      if (!src) { pageable_tables.resize(copy_bytes); src = pageable_tables.data(); }
      if (!copies.empty()) std::memcpy(src, copies.data(), copy_items_bytes);
      if (padded) std::memcpy(src + pad_off, pads.data(), pad_bytes);
      BATCH_CHECK(hipMemcpyAsync(t.copy_table, src, copy_bytes, hipMemcpyHostToDevice, s));
      if (!pinned) BATCH_CHECK(hipStreamSynchronize(s));  // (pageable source)
      launch_copy_table(s, static_cast<const CopyItem *>(t.copy_table), (long long)copies.size(), copy_max);
    } else {
      for (const CopyItem &c : copies) BATCH_CHECK(hipMemcpyAsync(c.dst, c.src, sizeof(double) * (size_t)c.words, kind, s));
    }
  }
  if (loc == AGP_HOST) BATCH_CHECK(hipStreamSynchronize(s));
  // information = L^-T z of every problem in ONE launch (solve.hip: backsub_coop_kernel, blockIdx.y = problem) for sizes
  // of few 128-row blocks: its output vectors are the hand-over buffers and enter sentinel-filled
  const bool coop = ctx->tune.backsub_coop && n <= ctx->tune.backsub_coop_max && g.nblk <= BACKSUB_DIRECT_BLOCKS;
  {
    PrepArgs prep;
    prep.fill(r.logsum, 0ull, 3 * g.cp2);  // log sums and flags
    if (coop) prep.sentinel(r.alpha, count * g.np2);
    launch_batch_prep(s, prep, g, r.invd, t.zpub);
  }
  {
    BatchGramTables gram(g, kernels, r.A, r.yvar, g.np2, r.flags, 4);
    for (int b = 0; b < count; ++b) {
      FeatView v = fits[(size_t)b]->train.v;
      if (padded) { v.sstride = n; v.n = features[b]->n; }  // the real rows of the padded features
      gram.set_view(b, v);
    }
    if ((st = launch_batch_grams(ctx, g, gram, kernels, t.gram_table, pinned ? pinned + gram_off : nullptr)) != AGP_OK) return fail(st);
  }
  if (padded)
    launch_ragged_pad(s, reinterpret_cast<const RaggedPadItem *>(static_cast<const char *>(t.copy_table) + pad_off), count, n, g.lda);
  factor_batch(ctx, g, /*allow_lookahead=*/true, r.A, r.invd, r.z, r.flags, 4, r.logsum, t.zpub);
  // information = L^-T (L^-1 y), gp.hpp:68
  if (coop) {
    backward_solve_coop(s, r.A, n, g.lda, r.invd, r.z, r.alpha, r.flags, nullptr, count, g.stride_A, g.stride_I, g.np2, g.np2, 4);
  } else {
    BATCH_CHECK(hipMemcpyAsync(r.alpha, r.z, sizeof(double) * (size_t)count * (size_t)g.np2, hipMemcpyDeviceToDevice, s));
    backward_solve_vec_batched(s, r.A, g.stride_A, n, g.lda, r.invd, g.stride_I, r.alpha, g.np2, count);
  }
  std::vector<double> h_log((size_t)g.cp2);
  std::vector<int> h_flags(4 * (size_t)count);
  BATCH_CHECK(hipMemcpyAsync(h_log.data(), r.logsum, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, s));
  BATCH_CHECK(hipMemcpyAsync(h_flags.data(), r.flags, sizeof(int) * 4 * (size_t)count, hipMemcpyDeviceToHost, s));
  BATCH_CHECK(hipStreamSynchronize(s));
  BATCH_CHECK(hipGetLastError());
  for (int b = 0; b < count; ++b)
    if (h_flags[4 * (size_t)b + 2]) {  // a hand-over of the one-launch substitution timed out (its producer died)
      ctx->last_error = "batched back substitution: hand-over timed out";
      return fail(AGP_ERR_HIP);
    }
  // the information vectors of the good fits go to the caller BEFORE any handle is published: a failed copy must not leave
  // the caller with an error code AND live handles (a failed problem leaves its column untouched)
  if (information)
    for (int b = 0; b < count; ++b) {
      const int *fl = &h_flags[4 * (size_t)b];
      if (!fl[0] && !fl[1])  // (the real rows: trailing phantom rows follow them)
        BATCH_CHECK(hipMemcpy(information + (size_t)b * (size_t)ldi, r.alpha + (size_t)b * (size_t)g.np2,
                              sizeof(double) * (size_t)features[b]->n, hipMemcpyDeviceToHost));
    }
  agp_fit_slab *slab = new (std::nothrow) agp_fit_slab();
  if (!slab) return fail(AGP_ERR_INVALID_ARGUMENT);
  slab->base = std::move(base);
  slab->bytes = bytes;
  slab->refs = count;
  for (int b = 0; b < count; ++b) {
    agp_fit *fit = fits[(size_t)b];
    fit->ctx = ctx;
    fit->slab = slab;
    fit->device = ctx->device;
    fit->n = n;
    fit->lda = g.lda;
    fit->A_bytes = sizeof(double) * (size_t)g.stride_A;
    fit->A = r.A + (size_t)b * (size_t)g.stride_A;
    fit->invd = r.invd + (size_t)b * (size_t)g.stride_I;
    fit->alpha = r.alpha + (size_t)b * (size_t)g.np2;
    fit->z = r.z + (size_t)b * (size_t)g.np2;
    if (features[b]->n < n) {  // (a pivot is a real row: the phantom rows come last and never fail)
      fit->n_real = features[b]->n;
      fit->phantom.emplace_back((long long)features[b]->n, n);
    }
    const int *fl = &h_flags[4 * (size_t)b];
    fit->failed_pivot = fl[1] ? (int64_t)fl[1] - 1 : -1;
    fit->log_det = 2. * h_log[(size_t)b];
    status[b] = fl[0] ? AGP_ERR_NAN_INPUT : (fl[1] ? AGP_ERR_NOT_POSITIVE_DEFINITE : AGP_OK);  // gp.hpp:66, then the factor
    fit->fail_status = status[b];
    if (log_det) log_det[b] = fit->log_det;
    out[b] = fit;
  }
#undef BATCH_CHECK
  return AGP_OK;
}

extern "C" {

int agp_fit_create_batch(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                         const double *y, int64_t ldy, const double *y_var, int64_t ldv, agp_fit **out, double *information,
                         int64_t ldi, double *log_det, int *status) {
  return fit_create_batch(c, count, kernels, features, y, ldy, y_var, ldv, out, information, ldi, log_det, status, false);
}

int agp_fit_create_batch_ragged(agp_context *c, int count, const agp_kernel *const *kernels, const agp_features *const *features,
                                const double *y, int64_t ldy, const double *y_var, int64_t ldv, agp_fit **out, double *information,
                                int64_t ldi, double *log_det, int *status) {
  return fit_create_batch(c, count, kernels, features, y, ldy, y_var, ldv, out, information, ldi, log_det, status, true);
}

int64_t agp_fit_padded_size(const agp_fit *fit) { return fit ? fit->n : 0; }

// ---- solve -----------------------------------------------------------------
int agp_solve(agp_context *ctx, const agp_fit *fit, const double *rhs, int64_t nrhs, double *out, int location) {
  if (!ctx || !fit || !rhs || !out || nrhs < 0) return AGP_ERR_INVALID_ARGUMENT;
  if (nrhs == 0) return AGP_OK;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const long long n = fit->n, ldb = round_up(n, 2);
  const hipMemcpyKind kind = location == AGP_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (!fit->phantom.empty()) {
    // rhs / out hold the REAL rows: spread them over the padded rows (phantom rows zero), solve, gather
    const long long nr = fit_real_rows(fit);
    DevMem<double> B;
    AGP_HIP_CHECK(ctx, B.alloc_plain(sizeof(double) * (size_t)ldb * (size_t)nrhs));
    int st = fit_expand_matrix(ctx, fit, rhs, nr, nrhs, B, ldb, location);
    if (st == AGP_OK) {
      forward_solve_mat_lookahead(ctx, fit->A, n, fit->lda, fit->invd, B, nrhs, ldb);
      backward_solve_mat(ctx->stream, fit->A, n, fit->lda, fit->invd, B, nrhs, ldb);
      st = fit_compact_matrix(ctx, fit, B, ldb, nrhs, out, nr, location);
    }
    (void)hipStreamSynchronize(ctx->stream);
    return st;
  }
  if (nrhs == 1 && n >= 1024) {
    // one right-hand side: the matrix kernels would run 2 N / 128 launches on a single column; the vector chains
    // (fused 128-row forward steps, blocked backward substitution) are 4x shorter (N = 16384: 11.3 -> 2.7 ms)
    const long long nblk = (n + NB - 1) / NB;
    const size_t wf = (size_t)nblk * NB * NB;
    int st1 = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * ((size_t)ldb + wf + backsolve_ws_elems(n)));
    if (st1 != AGP_OK) return st1;
    double *z = ctx->ws_aux, *Wfwd = z + ldb, *ws = Wfwd + wf;
    hipStream_t s = ctx->stream;
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(z, rhs, sizeof(double) * (size_t)n, kind, s));
    if (location == AGP_HOST) AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
    if (const long long BW = backsolve_width(n)) {
      // both directions through 512-wide inverted diagonal blocks (ws holds the backward solve's staging + inverses;
      // the inverses are shared)
      double *xs = ws, *W = ws + round_up(n, 2);
      invert_wide_blocks(s, fit->A, n, fit->lda, fit->invd, BW, W);
      forward_solve_vec_wide(s, fit->A, n, fit->lda, W, BW, z, xs);
      backward_solve_vec_wide(s, fit->A, n, fit->lda, W, BW, z, xs);
      return copy_out(ctx, z, n, out, location);
    }
    invert_diag_blocks_forward(s, n, fit->invd, Wfwd);
    forward_solve_vec(s, fit->A, n, fit->lda, Wfwd, z, ws);  // ws[0 : n] as the staging vector
    backward_solve_vec_any(s, fit->A, n, fit->lda, fit->invd, z, ws);
    return copy_out(ctx, z, n, out, location);
  }
  int st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (size_t)ldb * (size_t)nrhs);
  if (st != AGP_OK) return st;
  AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(ctx->ws_aux, sizeof(double) * (size_t)ldb, rhs, sizeof(double) * (size_t)n,
                                      sizeof(double) * (size_t)n, (size_t)nrhs, kind, ctx->stream));
  if (location == AGP_HOST) AGP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  forward_solve_mat_lookahead(ctx, fit->A, n, fit->lda, fit->invd, ctx->ws_aux, nrhs, ldb);
  backward_solve_mat(ctx->stream, fit->A, n, fit->lda, fit->invd, ctx->ws_aux, nrhs, ldb);
  return copy_out_2d(ctx, ctx->ws_aux, ldb, n, nrhs, out, n, location);
}

// ---- dense-matrix factor ---------------------------------------------------------
// copies the lower triangle of K into a fresh factor buffer and runs the LL^T;
// y (device, optional) receives the fused forward substitution (api_internal.h: also scores.hip's factor)
// diag_add (device, optional): n values added to the diagonal of the COPY before it is factored
int factor_dense(agp_context *c, const double *K, long long n, long long ld, int uplo, int location,
                 agp_fit *fit, double *y, const double *diag_add) {
  agp_context_impl *ctx = static_cast<agp_context_impl *>(c);
  hipStream_t s = ctx->stream;
  const long long nblk = (n + NB - 1) / NB;
  fit->ctx = ctx;
  fit->device = ctx->device;
  fit->n = n;
  fit->lda = factor_ld(n);
  fit->A_bytes = sizeof(double) * (size_t)fit->lda * (size_t)n;
  fit->own_A.adopt(static_cast<double *>(ctx->pool_A.take(fit->A_bytes)));
  if (!fit->own_A) AGP_HIP_CHECK(ctx, fit->own_A.alloc_cached(fit->A_bytes));
  fit->A = fit->own_A;
  AGP_HIP_CHECK(ctx, fit->own_part[0].alloc_cached(sizeof(double) * (size_t)nblk * (36 * MB * MB)));
  fit->invd = fit->own_part[0];
  const double *src = K;  // device-resident source of the triangle
  if (location == AGP_HOST) {
    // a pitched copy from pageable host memory degenerates into one small copy per
    // column; upload the matrix in one piece and re-pitch it on the device
    const size_t bytes = sizeof(double) * (size_t)ld * (size_t)n;
    int st = reserve_ws(ctx, ctx->ws_aux, bytes);
    if (st != AGP_OK) return st;
    AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->ws_aux, K, bytes - sizeof(double) * (size_t)(ld - n), hipMemcpyHostToDevice, s));
    src = ctx->ws_aux;
  }
  if (uplo == 0)
    AGP_HIP_CHECK(ctx, hipMemcpy2DAsync(fit->A, sizeof(double) * (size_t)fit->lda, src, sizeof(double) * (size_t)ld,
                                        sizeof(double) * (size_t)n, (size_t)n, hipMemcpyDeviceToDevice, s));
  else
    launch_upper_to_lower(s, src, ld, fit->A, fit->lda, n);
  AGP_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int), s));
  AGP_HIP_CHECK(ctx, hipMemsetAsync(ctx->d_scalars, 0, 4 * sizeof(double), s));
  if (diag_add) launch_add_diagonal(s, fit->A, fit->lda, n, diag_add);
  launch_nan_scan_lower(s, fit->A, fit->lda, n, ctx->d_flags);
  factor_lower(ctx, fit->A, n, fit->lda, fit->invd, y);
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_flags, ctx->d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  AGP_HIP_CHECK(ctx, hipStreamSynchronize(s));
  AGP_HIP_CHECK(ctx, hipGetLastError());
  fit->failed_pivot = ctx->h_flags[1] ? (int64_t)ctx->h_flags[1] - 1 : -1;
  fit->log_det = 2. * ctx->h_scalars[0];
  return status_from_flags(ctx);
}

int agp_factor_create(agp_context *ctx, const double *K, int64_t n, int64_t ld, int uplo, int location,
                      agp_fit **out) {
  if (!ctx || !K || !out || n <= 0 || ld < n || (uplo != 0 && uplo != 1)) return AGP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  agp_fit *fit = new (std::nothrow) agp_fit();
  if (!fit) return AGP_ERR_INVALID_ARGUMENT;
  const int st = factor_dense(ctx, K, n, ld, uplo, location, fit, nullptr);
  if (st == AGP_ERR_HIP) { agp_fit_destroy(fit); return st; }
  *out = fit;  // on NOT_POSITIVE_DEFINITE / NAN the handle only carries the failed pivot
  return st;
}

int agp_nll_dense(agp_context *ctx, const double *deviation, const double *K, int64_t n, int64_t ld, int uplo,
                  int location, double *out) {
  if (!ctx || !deviation || !K || !out || n <= 0 || ld < n || (uplo != 0 && uplo != 1)) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n == 1) {  // univariate shortcut, likelihood.hpp:57-60 -> -gaussian::log_pdf(deviation, variance)
    double d = 0., v = 0.;
    const hipMemcpyKind kind = location == AGP_HOST ? hipMemcpyHostToHost : hipMemcpyDeviceToHost;
    AGP_HIP_CHECK(ctx, hipMemcpy(&d, deviation, sizeof(double), kind));
    AGP_HIP_CHECK(ctx, hipMemcpy(&v, K, sizeof(double), kind));
    *out = 0.5 * (std::log(2 * M_PI * v) + d * d / v);
    return AGP_OK;
  }
  agp_fit *fit = new (std::nothrow) agp_fit();
  if (!fit) return AGP_ERR_INVALID_ARGUMENT;
  DevMem<double> z;
  hipError_t e = static_cast<hipError_t>(z.alloc_plain(sizeof(double) * (size_t)n));
  if (e != hipSuccess) { delete fit; ctx->last_error = hipGetErrorString(e); return AGP_ERR_HIP; }
  int st = vector_to_device(ctx, deviation, n, location, z);
  if (st == AGP_OK) st = factor_dense(ctx, K, n, ld, uplo, location, fit, z);
  if (st == AGP_OK) {
    launch_dot(ctx->stream, z, z, n, ctx->d_scalars + 1);  // dev^T K^-1 dev = z^T z
    e = hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); st = AGP_ERR_HIP; }
    else *out = 0.5 * (fit->log_det + ctx->h_scalars[1] + (double)n * std::log(2 * M_PI));
  }
  z.reset();  // (before the factor, as ever)
  agp_fit_destroy(fit);
  return st;
}

// ---- leave-one-out fast path ---------------------------------------------------
// diag(K^-1) into ws_aux[ldr * n ...]; returns the device pointer of the n results
static int inverse_diagonal_device(agp_context *ctx, const agp_fit *fit, double **diag_out) {
  const long long n = fit->n, ldr = factor_ld(n);
  const size_t r_elems = (size_t)ldr * (size_t)n;
  int st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (r_elems + 3 * (size_t)round_up(n, 2)));
  if (st != AGP_OK) return st;
  double *R = ctx->ws_aux, *diag = R + r_elems;
  hipStream_t s = ctx->stream;
  launch_set_identity(s, R, ldr, n);
  // R = L^-1 (serializable_ldlt.hpp:154-160), exploiting the triangular right-hand side
  forward_solve_mat_lookahead(ctx, fit->A, n, fit->lda, fit->invd, R, n, ldr, /*rhs_lower=*/true);
  // (K^-1)_ii = || R[:, i] ||^2   (sub_matrix^T * sub_matrix, :171-172)
  launch_coldot(s, R, ldr, R, ldr, n, n, diag, -1.0, nullptr);
  AGP_HIP_CHECK(ctx, hipGetLastError());
  *diag_out = diag;
  return AGP_OK;
}

int agp_fit_inverse_diagonal(agp_context *ctx, const agp_fit *fit, double *out, int out_location) {
  if (!ctx || !fit || !out || !fit->A) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  double *diag = nullptr;
  int st = inverse_diagonal_device(ctx, fit, &diag);
  if (st != AGP_OK) return st;
  if (!fit->phantom.empty()) return fit_compact_vector(ctx, fit, diag, out, out_location);
  return copy_out(ctx, diag, fit->n, out, out_location);
}

int agp_loo_marginal(agp_context *ctx, const agp_fit *fit, const double *y, double *mean, double *variance,
                     int location) {
  if (!ctx || !fit || !y || !mean || !variance || !fit->A || !fit->alpha) return AGP_ERR_INVALID_ARGUMENT;
  if (!fit->phantom.empty()) return AGP_ERR_UNSUPPORTED;  // cross validation of a fit grown by agp_fit_update: refit instead
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const long long n = fit->n;
  double *diag = nullptr;
  int st = inverse_diagonal_device(ctx, fit, &diag);
  if (st != AGP_OK) return st;
  double *yd = diag + round_up(n, 2), *md = yd + round_up(n, 2);  // mean overwrites... separate slots below
  if ((st = vector_to_device(ctx, y, n, location, yd)) != AGP_OK) return st;
  // variance is written over the diag slot's successor: reuse `diag` for the variance after reading it
  launch_loo(ctx->stream, diag, yd, fit->alpha, n, md, diag);
  if ((st = copy_out(ctx, md, n, mean, location)) != AGP_OK) return st;
  return copy_out(ctx, diag, n, variance, location);
}

// ---- predict ---------------------------------------------------------------
int agp_predict_mean(agp_context *ctx, const agp_kernel *k, const agp_fit *fit, const agp_features *xs,
                     double *mean, int out_location) {
  if (!ctx || !k || !fit || !xs || !mean) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(xs);
  if (st != AGP_OK) return st;
  if (!fit->alpha || xs->dim != fit->train.v.dim) return AGP_ERR_INVALID_ARGUMENT;
  const long long m = xs->n;
  if (m == 0) return AGP_OK;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dxs;
  if ((st = to_device(ctx, xs, false, &dxs)) != AGP_OK) return st;
  // cross_cov = cov(train_features, features); mean = cross_cov^T information  (gp.hpp:361-363)
  if (out_location == AGP_DEVICE) {  // straight into the caller's buffer: no staging copy
    launch_predict_mean(ctx->stream, dprog, fit->train.v, dxs.v, fit->alpha, mean, &k->prog);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->last_error = "agp_predict_mean: stream"; st = AGP_ERR_HIP; }
  } else {
    st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (size_t)m);
    if (st == AGP_OK) {
      launch_predict_mean(ctx->stream, dprog, fit->train.v, dxs.v, fit->alpha, ctx->ws_aux, &k->prog);
      st = copy_out(ctx, ctx->ws_aux, m, mean, out_location);
    }
  }
  dxs.release();
  return st;
}

// rows [o, o + cnt) of a device feature view (scale columns keep the stride of the whole vector)
static FeatView feature_range(const FeatView &v, long long o, long long cnt) {
  FeatView r = v;
  r.sstride = scale_stride(v);
  r.n = cnt;
  r.coords = v.coords + o * v.dim;
  r.ids = v.ids ? v.ids + o : nullptr;
  r.scales = v.scales ? v.scales + o : nullptr;
  return r;
}

// Test points per pass of a marginal prediction: the n x m block L^-1 K* is the only large buffer, and nothing couples
// the columns of a marginal prediction, so m is cut into passes that keep it at 2 GiB (AGP_PREDICT_CHUNK=<points>
// overrides; a joint prediction needs all columns at once).
static long long marginal_chunk(const agp_context *ctx, long long rows) {
  if (ctx->tune.predict_chunk > 0) return ctx->tune.predict_chunk;
  const long long c = (1LL << 28) / (rows > 0 ? rows : 1);
  return c < 1024 ? 1024 : (c > (1LL << 20) ? (1LL << 20) : c);  // (a million points: the Gram kernels' grids stay in range)
}

static int predict_common(agp_context *ctx, const agp_kernel *k, const agp_fit *fit, const agp_features *xs,
                          double *mean, double *var_or_cov, bool joint, int out_location) {
  if (!ctx || !k || !fit || !xs || !mean || !var_or_cov) return AGP_ERR_INVALID_ARGUMENT;
  AGP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int st = validate_features(xs);
  if (st != AGP_OK) return st;
  if (!fit->alpha || xs->dim != fit->train.v.dim) return AGP_ERR_INVALID_ARGUMENT;
  const long long m_all = xs->n, n = fit->n;
  if (m_all == 0) return AGP_OK;
  const DevProgram *dprog = nullptr;
  if ((st = device_program(ctx, k, &dprog)) != AGP_OK) return st;
  DeviceFeatures dxs;
  if ((st = to_device(ctx, xs, false, &dxs)) != AGP_OK) return st;
  TraceRange tr_predict(joint ? "agp: predict joint (gp.hpp:103-113)" : "agp: predict marginal (gp.hpp:87-101)");
  const long long ldv = round_up(n, 2);
  const long long chunk = joint ? m_all : std::min(m_all, marginal_chunk(ctx, ldv));
  // workspace: V (n x chunk) | mean (chunk) | prior (chunk, or m x m for a joint prediction)
  const long long ldc = round_up(chunk, 2);
  const size_t v_elems = (size_t)ldv * (size_t)chunk;
  const size_t p_elems = joint ? (size_t)ldc * (size_t)chunk : (size_t)ldc;
  st = reserve_ws(ctx, ctx->ws_aux, sizeof(double) * (v_elems + (size_t)ldc + p_elems));
  if (st != AGP_OK) { dxs.release(); return st; }
  double *V = ctx->ws_aux, *mean_d = V + v_elems, *prior = mean_d + ldc;
  hipStream_t s = ctx->stream;
  for (long long o = 0; o < m_all && st == AGP_OK; o += chunk) {
    const long long m = std::min(chunk, m_all - o);
    const FeatView xv = (o == 0 && m == m_all) ? dxs.v : feature_range(dxs.v, o, m);
    // mean (gp.hpp:82-85)
    launch_predict_mean(s, dprog, fit->train.v, xv, fit->alpha, mean_d, &k->prog);
    // cross_cov = cov(train_features, features)   (gp.hpp:316,337)
    launch_gram(s, dprog, fit->train.v, xv, false, false, V, ldv, nullptr, nullptr, &k->prog);
    fit_zero_phantom_rows(s, fit, V, ldv, m);
    // V = L^-1 K*  ;  explained = V^T V  (== K*^T K^-1 K*, gp.hpp:96,111)
    if (m == 1 && n >= 1024) {
      // a single test point: the vector chain (one fused launch per 128 rows) instead of the matrix kernels
      const long long nblk = (n + NB - 1) / NB;
      DevMem<double> Wfwd;
      const long long BWp = backsolve_width(n);
      const size_t w_elems = BWp ? (size_t)(n / BWp) * (size_t)BWp * (size_t)BWp : (size_t)nblk * NB * NB;
      if (Wfwd.alloc_plain(sizeof(double) * (w_elems + (size_t)round_up(n, 2))) != 0) {
        dxs.release();
        ctx->last_error = "hipMalloc (single-point prediction workspace)";
        return AGP_ERR_HIP;
      }
      double *stage = Wfwd + w_elems;
      if (BWp) {  // through 512-wide inverted diagonal blocks (see agp_solve)
        invert_wide_blocks(s, fit->A, n, fit->lda, fit->invd, BWp, Wfwd);
        forward_solve_vec_wide(s, fit->A, n, fit->lda, Wfwd, BWp, V, stage);
      } else {
        invert_diag_blocks_forward(s, n, fit->invd, Wfwd);
        forward_solve_vec(s, fit->A, n, fit->lda, Wfwd, V, stage);
      }
      (void)hipStreamSynchronize(s);
    } else {
      forward_solve_mat_lookahead(ctx, fit->A, n, fit->lda, fit->invd, V, m, ldv);
    }
    if (!joint) {
      launch_gram_diagonal(s, dprog, xv, prior);                      // gp.hpp:339-343
      launch_coldot(s, V, ldv, V, ldv, n, m, prior, 1.0, prior);      // gp.hpp:97-99
      st = copy_out(ctx, mean_d, m, mean + o, out_location);
      if (st == AGP_OK) st = copy_out(ctx, prior, m, var_or_cov + o, out_location);
    } else {
      launch_gram(s, dprog, xv, xv, true, false, prior, ldc, nullptr, nullptr, &k->prog);  // prior_cov, gp.hpp:317
      launch_gemm_nt_sub(s, prior, ldc, V, ldv, true, V, ldv, true, m, m, n, true);   // lower tiles
      launch_symmetrize(s, prior, ldc, m);
      st = copy_out(ctx, mean_d, m, mean, out_location);
      if (st == AGP_OK) st = copy_out_2d(ctx, prior, ldc, m, m, var_or_cov, m, out_location);
    }
  }
  dxs.release();
  return st;
}

int agp_predict_marginal(agp_context *ctx, const agp_kernel *k, const agp_fit *fit, const agp_features *xs,
                         double *mean, double *variance, int out_location) {
  return predict_common(ctx, k, fit, xs, mean, variance, false, out_location);
}

int agp_predict_joint(agp_context *ctx, const agp_kernel *k, const agp_fit *fit, const agp_features *xs,
                      double *mean, double *cov, int out_location) {
  return predict_common(ctx, k, fit, xs, mean, cov, true, out_location);
}

}  // extern "C"
