// The library's own state and bookkeeping behind the C ABI (include/xnrs_hip.h): version, build id, error and status
// strings, the development knobs, the forward-GEMM mode and the launch timer.  Every other extern "C" entry point sits
// beside the code it drives: encoder_fwd.hip (the three forward pipelines, the fold), encoder_bwd.hip (training forward
// and backward, linear backward), scorers.hip, infonce.hip, batch.hip, gather.hip, row_lists.hip, pool_score.hip /
// pool_bwd.hip (dot scoring), personalized.hip; host.h holds what they share.
//
// No entry point allocates device memory or synchronises: everything is enqueued on the caller's stream into the
// caller's workspace (hipGraph-capturable) -- or, for the backward's weight gradients, on a side stream forked from and
// joined back into the caller's stream inside the call (encoder_bwd.hip: SideLane).  Process-global state, none of it
// touched by a plain encode / score call:
//   - the forward-GEMM arithmetic mode (xnrs_set_gemm_mode, an atomic int) and the development knobs (read once at load,
//     xnrs_reload_knobs): gemm_f32.hip;
//   - the optional launch timer (xnrs_profile_*, mutex-guarded, off by default): here; host.h's ProfScope only tests its mask;
//   - the backward's side stream and events, one set per device (mutex-guarded): encoder_bwd.hip;
//   - the caller's sticky status word (xnrs_set_status_word): here, read by the launchers through status_word().
#include <atomic>
#include <mutex>
#include <vector>

#include "host.h"

using namespace xnrs;

// ---- optional per-launch event timing (measurement aid; see xnrs_profile_enable in the header)
namespace xnrs {
uint32_t g_prof_mask = 0;  // 0 (default): ProfScope is a single load and compare
}
namespace {
std::vector<ProfRec> g_prof;
std::mutex g_prof_mu;      // guards g_prof / g_prof_mask changes; taken only while the timer is on
constexpr size_t PROF_MAX = 1 << 16;
}  // namespace

bool xnrs::prof_begin(ProfRec* r, hipStream_t stream) {
  if (hipEventCreate(&r->beg) != hipSuccess || hipEventCreate(&r->end) != hipSuccess) return false;
  (void)hipEventRecord(r->beg, stream);
  return true;
}

void xnrs::prof_end(const ProfRec& r, hipStream_t stream) {
  (void)hipEventRecord(r.end, stream);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_prof.size() < PROF_MAX) g_prof.push_back(r);
  else {
    (void)hipEventDestroy(r.beg);
    (void)hipEventDestroy(r.end);
  }
}

int64_t xnrs::prof_count(int stage, const int64_t* cnt, int which, int64_t host_value, hipStream_t stream) {
  if (!cnt || !prof_on(stage)) return host_value;
  int64_t v = host_value;
  if (hipStreamSynchronize(stream) != hipSuccess) return host_value;
  if (hipMemcpy(&v, cnt + which, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return host_value;
  return v;
}

// ---- the caller's sticky status word (kernels.h)
// ONE word, on the device that was current when it was registered: a launch on another device gets nullptr (its kernels must
// not be handed a pointer into this device's memory; their NaN outputs remain the signal there)
static std::atomic<int32_t*> g_status_word{nullptr};
static std::atomic<int> g_status_device{-1};
int32_t* xnrs::status_word() {
  int32_t* w = g_status_word.load(std::memory_order_relaxed);
  if (!w) return nullptr;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != g_status_device.load(std::memory_order_relaxed)) return nullptr;
  return w;
}
void xnrs::set_status_word(int32_t* w) {
  int dev = -1;
  (void)hipGetDevice(&dev);
  g_status_device.store(w ? dev : -1, std::memory_order_relaxed);
  g_status_word.store(w, std::memory_order_relaxed);
}

extern "C" {

int32_t xnrs_abi_version(void) { return XNRS_ABI_VERSION; }

#ifndef XNRS_BUILD_ID
#define XNRS_BUILD_ID "unknown"
#endif
const char* xnrs_build_id(void) { return XNRS_BUILD_ID; }

int32_t xnrs_set_status_word(int32_t* device_word) {
  set_status_word(device_word);
  return XNRS_OK;
}

const char* xnrs_status_string(int32_t word) {
  if (word == XNRS_STATUS_QUERY_RANGE)
    return "a query row index or user id outside its table (personalized attention: NaN outputs / clamped user ids)";
  if (word & XNRS_STATUS_QUERY_RANGE)
    return "several status bits: a query row index or user id out of range, and a bad mask value or table row id";
  switch (word & 3) {
    case 0: return "ok";
    case XNRS_STATUS_NONBINARY_MASK: return "a mask value other than 0 / 1 reached the device-compacted encoder (its outputs are NaN)";
    case XNRS_STATUS_ROW_RANGE: return "a news-table row id outside the table (clamped; the gathered rows are wrong)";
    default: return "a mask value other than 0 / 1 reached the device-compacted encoder AND a table row id was out of range";
  }
}

const char* xnrs_error_string(int32_t code) {
  switch (code) {
    case XNRS_OK: return "ok";
    case XNRS_EINVAL: return "invalid argument (shape or NULL pointer)";
    case XNRS_EHEADS: return "d_model is not divisible by n_heads";
    case XNRS_EWORKSPACE: return "workspace too small";
    case XNRS_EUNSUPPORTED:
      return "shape outside the supported range (attention S <= 128, pooling N <= 512, head width d_k <= 128, "
             "personalized attention L <= 4096, CAUM pooling H <= 8192)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

int32_t xnrs_set_gemm_mode(int32_t mode) {
  const int prev = xnrs::gemm_mode();
  xnrs::set_gemm_mode(mode);
  return prev;
}

int32_t xnrs_get_gemm_mode(void) { return xnrs::gemm_mode(); }

int32_t xnrs_train_fold_enabled(void) { return fold_wanted(knobs().fold_train) ? 1 : 0; }

int32_t xnrs_reload_knobs(void) {
  xnrs::reload_knobs();
  return XNRS_OK;
}

int32_t xnrs_qkv_launch_count(int32_t reset) {
  const int64_t n = xnrs::qkv_launches_read(reset != 0);
  return n > 0x7fffffffLL ? 0x7fffffff : (int32_t)n;
}

int32_t xnrs_qkv_one_launch_map(int64_t block, int64_t live_tiles, int64_t live_rows, int32_t kv_row_tiles, int32_t kv_col_tiles,
                                int64_t q_rows, int32_t q_tile_rows, int32_t q_col_tiles, int32_t* section, int32_t* index) {
  if (kv_row_tiles < 0 || kv_col_tiles < 1 || q_rows < 0 || q_tile_rows < 1 || q_col_tiles < 1) return XNRS_EINVAL;
  const int64_t grid = xnrs::qkv_one_launch_grid(kv_row_tiles, kv_col_tiles, q_rows, q_tile_rows, q_col_tiles);
  if (grid > 0x7fffffffLL) return XNRS_EINVAL;
  if (section && index) {
    const xnrs::QkvOneLaunchWork w =
        xnrs::qkv_one_launch_map(block, live_tiles, live_rows, kv_row_tiles, kv_col_tiles, q_rows, q_tile_rows, q_col_tiles);
    *section = w.section;
    *index = w.index;
  }
  return (int32_t)grid;
}

int32_t xnrs_fc1_in_tail_count(int32_t reset) {
  const int64_t n = xnrs::fc1_in_tail_read(reset != 0);
  return n > 0x7fffffffLL ? 0x7fffffff : (int32_t)n;
}

int32_t xnrs_mha_live_o_count(int32_t reset) {
  const int64_t n = xnrs::mha_live_o_read(reset != 0);
  return n > 0x7fffffffLL ? 0x7fffffff : (int32_t)n;
}

int32_t xnrs_qkv_fc1_launch_map(int64_t block, int64_t live_tiles, int64_t live_rows, int64_t fc1_live_rows, int32_t kv_row_tiles,
                                int32_t kv_col_tiles, int64_t q_rows, int32_t q_tile_rows, int32_t q_col_tiles, int64_t fc1_rows,
                                int32_t fc1_tile_rows, int32_t fc1_col_tiles, int32_t* section, int32_t* index) {
  if (kv_row_tiles < 0 || kv_col_tiles < 1 || q_rows < 0 || q_tile_rows < 1 || q_col_tiles < 1 || fc1_rows < 0 || fc1_tile_rows < 1 ||
      fc1_col_tiles < 1)
    return XNRS_EINVAL;
  const int64_t grid =
      xnrs::qkv_fc1_launch_grid(kv_row_tiles, kv_col_tiles, q_rows, q_tile_rows, q_col_tiles, fc1_rows, fc1_tile_rows, fc1_col_tiles);
  if (grid > 0x7fffffffLL) return XNRS_EINVAL;
  if (section && index) {
    const xnrs::QkvOneLaunchWork w = xnrs::qkv_fc1_launch_map(block, live_tiles, live_rows, fc1_live_rows, kv_row_tiles, kv_col_tiles, q_rows,
                                                              q_tile_rows, q_col_tiles, fc1_rows, fc1_tile_rows, fc1_col_tiles);
    *section = w.section;
    *index = w.index;
  }
  return (int32_t)grid;
}

int32_t xnrs_profile_enable(uint32_t stage_mask) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) {
    (void)hipEventDestroy(r.beg);
    (void)hipEventDestroy(r.end);
  }
  g_prof.clear();
  g_prof_mask = stage_mask;
  return XNRS_OK;
}

int32_t xnrs_profile_read(double* ms, int64_t* launches, double* flops) {
  if (!ms || !launches || !flops) return XNRS_EINVAL;
  for (int i = 0; i < XNRS_PROFILE_STAGES; ++i) {
    ms[i] = 0.0;
    launches[i] = 0;
    flops[i] = 0.0;
  }
  int32_t rc = XNRS_OK;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) {
    float t = 0.f;
    hipError_t e = hipEventSynchronize(r.end);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, r.beg, r.end);
    if (e != hipSuccess) rc = (int32_t)e;
    else {
      ms[r.stage] += t;
      launches[r.stage] += 1;
      flops[r.stage] += r.flops;
    }
    (void)hipEventDestroy(r.beg);
    (void)hipEventDestroy(r.end);
  }
  g_prof.clear();
  return rc;
}

}  // extern "C"
