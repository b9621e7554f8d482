// afe_consumer.h -- host plumbing shared by the library's consumers of the engine's device state and by the perception
// entry points: depth camera (afe_render.hip), planner API (afe_planner_api.cpp), clearance query, contact monitor and path
// audit (afe_clearance.hip), ensemble statistics (afe_stats.hip), trajectory follower (afe_follower.hip), mocap estimator (afe_estimator.hip), flight stage machine (afe_stages.hip), onboard flight computer (afe_onboard.hip).  Internal to the library, host only, header only.
//
//   engine_stream_device / engine_device_view / engine_shard   the engine's entry points for the library's other translation
//                        units (implemented in afe_engine.cpp; afe_world.hip and afe_comm.cpp use the first and the last alone)
//   pick_gfx950          the device a create call runs on: the given one or the current one, refused unless it is a gfx950
//   DevBuf / PinnedBuf   device / pinned host memory that lives as long as its owner: a scope, or a handle (afe_devmem.h)
//   StreamTimer          two events round the launches of a call; without timing it is nothing and synchronises nothing
//   engine_enter         the ONE way a consumer gets at the engine: stream, device and view, the device made current
//   engine_range_bad     [first, first + count) against the engine's size, nothing touched
//
// ORDER OF REFUSALS at an entry that consumes an engine.  First the call's own arguments (AFE_ERR_INVALID_ARG, then
// AFE_ERR_OUT_OF_RANGE), then the range against the engine's size (engine_range_bad) and the empty request -- answered
// AFE_OK before the engine is touched, so an audit of nothing does not end a resident grid -- then engine_enter: it passes
// the engine's gate (a resident grid ends here, a failed engine refuses with the status of its first failure), then
// hipSetDevice (AFE_ERR_HIP).  Only THEN the consumer compares its own handle with what it got (a map or scene on another
// device, a monitor made for another vehicle count: AFE_ERR_INVALID_ARG).  So a call that is wrong in two ways at once -- a
// failed engine AND a handle on another device -- reports the engine.  afe_render_depth_engine alone takes the range from
// the view and therefore enters first: engine, range, empty request, device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "../../include/agrifly_engine.h"
#include "afe_devmem.h"

namespace afe {

// implemented in afe_engine.cpp: the stream the engine launches on and its device
void engine_stream_device(afe_engine *e, void **stream, int *device);
// afe_get_device_view for the library's own consumers (the slabs do not leave the engine: afe_sync keeps its short form)
int engine_device_view(afe_engine *e, struct afe_device_view *out);
// afe_engine.cpp: the engine's size, nothing touched
void engine_shard(const afe_engine *e, int64_t *first_global, int64_t *n);
// afe_engine.cpp: the slabs afe_set_rates_commands writes (4 planar floats and one byte per vehicle, the engine's stride), for
// the follower, which delivers on the device what that call uploads.  AFE_ERR_NOT_CONFIGURED without afe_set_rates_logic.
// The caller has passed the gate (engine_enter) and launches on the engine's stream.
int engine_rates_slabs(afe_engine *e, float **rates_cmd, uint8_t **have_cmd);
// afe_engine.cpp: what rates_logic_tick keeps, for the GPS + IMU estimator, which consumes the logic's own filtered gyro
// (LowPassFilterSecondOrder::GetValue is ym1: rows 9-11 of *lpf, 12 planar floats with the engine's stride) and rotates the
// accelerometer sample by the logic's mount matrix (logic_table[type].R, device memory, current after the last afe_step);
// *period = float(logic period), *n_ticks = afe_logic_ticks.  AFE_ERR_NOT_CONFIGURED without afe_set_rates_logic.  The
// caller has passed the gate and launches on the engine's stream.
struct DevLogic;
int engine_logic_filter(afe_engine *e, const float **lpf, const DevLogic **logic_table, float *period, uint64_t *n_ticks);
// afe_engine.cpp: the clock of the latest logic tick for the onboard flight computer (afe_onboard.hip), which runs behind the step
// that fired it.  *tick_start_us: the engine clock at the START of that step (the reference's logic reads the master clock inside
// Quadcopter_T::Run, before main.cpp:392 advances it); *steps_after: steps issued since that step.  The caller has passed the gate.
int engine_tick_clock(afe_engine *e, uint64_t *tick_start_us, uint64_t *steps_after);
// THE RADIO MAILBOX: per-vehicle words of an onboard computer's handle (the engine's stride) that say which vehicles were handed
// a radio message since its last tick: arrival time + 1 (0: none), RadioTypes type, flags.  The engine holds a BORROWED pointer
// to them while an onboard computer exists (all NULL otherwise: then nothing changes for anybody).  Every place that delivers a
// command stamps it: afe_set_rates_commands, afe_set_commands_from_radio, the follower's and the stage machine's tick.
struct RadioMailbox {
  unsigned long long *arrival;
  uint8_t *type, *flags;
};
// afe_engine.cpp: records in the vehicle type table (a consumer's per-type table pairs with it)
int engine_type_records(const afe_engine *e);
// afe_engine.cpp: m == NULL withdraws; a second onboard computer on one engine is AFE_ERR_INVALID_ARG
int engine_set_mailbox(afe_engine *e, const RadioMailbox *m);
void engine_mailbox(const afe_engine *e, RadioMailbox *m);
// afe_onboard.hip: stamp vehicles [first, first + count) on `stream`: arrival = now_us + 1; type >= 0: that type and flags 0 for
// all; dev_types != NULL (a device row of the engine's stride, indexed by vehicle): each vehicle's own type, flags 0, and a
// vehicle whose type is 0 was handed nothing and is left alone; type < 0 and no row: the arrival time alone.  m.arrival == NULL: nothing.
int onboard_stamp(void *stream, const RadioMailbox &m, int64_t first, int64_t count, uint64_t now_us, int type, const uint8_t *dev_types);
// afe_engine.cpp: AFE_ERR_INVALID_ARG for an engine whose state is host-visible (its setters go round the stream), for the
// estimator, which like the follower works on the stream alone.  The caller has passed the gate.
int engine_device_resident(afe_engine *e);

// afe_planner_api.cpp: afe_rappids_plan_device for a caller whose planner inputs are in device memory already (planar [3][n]
// doubles on `device`) and who takes the plans over there.  Nothing but the candidate table is uploaded; `out` and `flags`
// are downloaded only where they are not NULL.  adopt(ctx, dev_out) runs after the planner's kernels have finished and while
// the call still holds the planner's scratch: dev_out[n] is valid until it returns.
struct PlanDeviceIO {
  const double *vel0, *acc0, *grav, *cost_vec;
  int (*adopt)(void *ctx, const afe_plan_output *dev_out);
  void *ctx;
};
int plan_device_resident(int device, const afe_planner_config *cfg, int64_t n, const void *dev_depth_images, const double *samples,
                         int n_candidates, const PlanDeviceIO &io, afe_plan_output *out, uint8_t *flags, float *kernel_ms);

inline int pick_gfx950(int device, int *out) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return AFE_ERR_NO_DEVICE;
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return AFE_ERR_NO_DEVICE;
  if (device >= n_dev) return AFE_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return AFE_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return AFE_ERR_HIP;
  *out = device;
  return AFE_OK;
}

// hipMalloc / hipFree, and pinned host memory with the flags of its one kind of use (afe_devmem.h: the owner and its rules).
// A refusal is taken off the runtime -- which keeps a thread's last error until somebody reads it -- and kept here for whoever
// wants its text: a request granted at the second attempt (reserve's fallback) leaves no error behind for the launches after it.
inline hipError_t &last_refusal() { static thread_local hipError_t e = hipSuccess; return e; }
inline void *granted(hipError_t status, void *p) {
  if (status == hipSuccess) return p;
  (void)hipGetLastError();
  last_refusal() = status;
  return nullptr;
}
struct DeviceMemory {
  static void *get(size_t bytes) { void *p = nullptr; return granted(hipMalloc(&p, bytes), p); }
  static void put(void *p) { (void)hipFree(p); }
};
template <unsigned FLAGS>
struct PinnedMemory {
  static void *get(size_t bytes) { void *p = nullptr; return granted(hipHostMalloc(&p, bytes, FLAGS), p); }
  static void put(void *p) { (void)hipHostFree(p); }
};
template <unsigned FLAGS = hipHostMallocDefault>
using PinnedBuf = OwnedBuf<PinnedMemory<FLAGS>>;

struct DevBuf : OwnedBuf<DeviceMemory> {
  bool upload(const void *src, size_t bytes) { return alloc(bytes) && hipMemcpy(get(), src, bytes, hipMemcpyHostToDevice) == hipSuccess; }
  bool download(void *host, size_t bytes) const { return hipMemcpy(host, get(), bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};

// The start event is recorded on construction; finish() goes behind the last launch.  Untimed: no event, no record, no wait.
struct StreamTimer {
  hipStream_t stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool timed;
  StreamTimer(hipStream_t stream_, bool timed_) : stream(stream_), timed(timed_) {
    if (timed && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) (void)hipEventRecord(e0, stream);
  }
  StreamTimer(const StreamTimer &) = delete;
  StreamTimer &operator=(const StreamTimer &) = delete;
  ~StreamTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  bool ok() const { return !timed || e1 != nullptr; }      // false: an event could not be made -- launch nothing, AFE_ERR_HIP
  // the launches' status in, the call's status out; waits for the launches only if they went out, then *ms = their time
  int finish(int status, float *ms) {
    if (!timed) return status;
    if (!ok()) return AFE_ERR_HIP;
    (void)hipEventRecord(e1, stream);
    if (status == AFE_OK && hipEventSynchronize(e1) != hipSuccess) status = AFE_ERR_HIP;
    if (status == AFE_OK) (void)hipEventElapsedTime(ms, e0, e1);
    return status;
  }
};

struct EngineAccess {
  hipStream_t stream;
  int device;
  afe_device_view view;
};

// (see ORDER OF REFUSALS above)
inline int engine_enter(afe_engine *e, EngineAccess *a) {
  a->stream = nullptr;
  a->device = 0;
  engine_stream_device(e, (void **)&a->stream, &a->device);
  a->view.struct_bytes = sizeof(a->view);
  const int rc = engine_device_view(e, &a->view);
  if (rc != AFE_OK) return rc;
  return hipSetDevice(a->device) == hipSuccess ? AFE_OK : AFE_ERR_HIP;
}

inline bool engine_range_bad(const afe_engine *e, int64_t first, int64_t count) {
  int64_t first_global = 0, n = 0;
  engine_shard(e, &first_global, &n);
  return first > n || count > n - first;   // (no sum: it can wrap)
}

}  // namespace afe
