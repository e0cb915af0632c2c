// Directional rain-streak removal (csrc/derain.hip): what the chain of
// csrc/preprocess.hip needs to check, size and launch the op.
#pragma once
#include "common.h"

namespace rv {

// The normalised parameters of rv_streak_derain_u8 (include/rvhip.h).
struct StreakParams {
  int width, min_len, max_len, slant, thr;
};

// RV_EINVAL with a message for a parameter out of range (`what` names the
// caller in the message).
int streak_check(const StreakParams& p, const char* what);

// Workspace bytes; the arguments are already checked.
size_t streak_ws_bytes(int B, int H, int W, int max_len);

// in -> out.  flags: nullptr, or the chain gate's per-frame flags (frames it
// passed through are skipped).  s_out: nullable.
void launch_streak(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                   const StreakParams& p, void* ws, uint8_t* s_out, const int* flags,
                   hipStream_t s);

}  // namespace rv
