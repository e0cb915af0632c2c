// Live conv timing of YOLOv8 forwards: the rv_yolo_profile* entries set it up
// and read it back; the forward records the events (Profile::timed).
#include "yolo_model.h"

namespace rv {

int Profile::reset(int max_forwards, int slots, int reps_) {
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);  // teardown
  ev.clear();
  on = false;
  reps = reps_;
  n_fwd = 0;
  cap_fwd = max_forwards;
  per_fwd = slots;
  flops.assign(per_fwd, 0.0);
  bytes.assign(per_fwd, 0.0);
  conv_of.assign(per_fwd, -1);
  const size_t need = (size_t)cap_fwd * per_fwd * 2;
  for (ev.reserve(need); ev.size() < need;) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) {
      set_error("hipEventCreate failed");
      return RV_EINVAL;
    }
    ev.push_back(e);
  }
  on = max_forwards > 0;
  return RV_OK;
}

}  // namespace rv

using namespace rv;

extern "C" int rv_yolo_profile_reps(void* h, int max_forwards, int reps) {
  RV_CHECK_ARG(h && max_forwards >= 0 && reps >= 1, "bad args");
  Model* M = (Model*)h;
  return M->prof.reset(max_forwards, (int)M->def.convs.size(), reps);
}

extern "C" int rv_yolo_profile(void* h, int max_forwards) {
  return rv_yolo_profile_reps(h, max_forwards, 1);
}

// After the profiled forwards (synchronises): per conv launch index i,
// ms[i] = total device time over the recorded forwards, flops[i] =
// algorithmic FLOPs of ONE launch, conv[i] = conv spec index.  Returns the
// number of recorded forwards.
extern "C" int rv_yolo_profile_read(void* h, double* ms, double* flops, int* conv, int n) {
  RV_CHECK_ARG(h && ms && flops && conv, "bad args");
  Model* M = (Model*)h;
  Profile& P = M->prof;
  if (!P.on) return 0;
  for (int i = 0; i < n && i < P.per_fwd; ++i) {
    double tot = 0.0;
    for (int f = 0; f < P.n_fwd; ++f) {
      float t = 0.f;
      hipEvent_t a = P.event(f, i, 0), b = P.event(f, i, 1);
      if (P.conv_of[i] >= 0 && hipEventSynchronize(b) == hipSuccess &&
          hipEventElapsedTime(&t, a, b) == hipSuccess)
        tot += t;
    }
    ms[i] = tot / P.reps;
    flops[i] = P.flops[i];
    conv[i] = P.conv_of[i];
  }
  return P.n_fwd;
}

// After the profiled forwards (synchronises): the [start, end) interval of
// every recorded conv launch of handle h, in ms after the first recorded
// event of handle `ref` (forward 0; ref may be h).  Handles of one device
// share the clock, so the intervals of several forward contexts (lanes)
// can be merged into the chip-wide busy time of the conv family.  Writes
// at most n pairs; returns the number of intervals.
extern "C" int rv_yolo_profile_times(void* h, void* ref, double* t0, double* t1, int n) {
  RV_CHECK_ARG(h && ref && (n == 0 || (t0 && t1)), "bad args");
  Model* M = (Model*)h;
  const Profile& P = M->prof;
  const Profile& R = ((Model*)ref)->prof;
  if (!P.on || !R.on || R.n_fwd == 0) return 0;
  hipEvent_t e0 = nullptr;
  for (int i = 0; i < R.per_fwd && !e0; ++i)
    if (R.conv_of[i] >= 0) e0 = R.event(0, i, 0);
  if (!e0) return 0;
  int k = 0;
  for (int f = 0; f < P.n_fwd; ++f)
    for (int i = 0; i < P.per_fwd; ++i) {
      if (P.conv_of[i] < 0) continue;
      hipEvent_t a = P.event(f, i, 0), b = P.event(f, i, 1);
      float ta = 0.f, tb = 0.f;
      if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ta, e0, a) != hipSuccess ||
          hipEventElapsedTime(&tb, e0, b) != hipSuccess) {
        (void)hipGetLastError();
        set_error("rv_yolo_profile_times: event query failed");
        return RV_EINVAL;
      }
      if (k < n) {
        t0[k] = ta;
        t1[k] = tb;
      }
      ++k;
    }
  return k;
}

// Algorithmic HBM bytes of each conv launch of the profiled forwards (same
// indexing as rv_yolo_profile_read); returns the number of entries written.
extern "C" int rv_yolo_profile_bytes(void* h, double* bytes, int n) {
  RV_CHECK_ARG(h && bytes, "bad args");
  Model* M = (Model*)h;
  const Profile& P = M->prof;
  int k = 0;
  for (; k < n && k < (int)P.bytes.size(); ++k) bytes[k] = P.bytes[k];
  return k;
}
