// Dark-channel-prior dehaze (csrc/dehaze.hip): what the chain of
// csrc/preprocess.hip needs to check, size and launch the op.
#pragma once
#include "common.h"

namespace rv {

// The normalised parameters of rv_dcp_dehaze_u8 (include/rvhip.h).
struct DcpParams {
  int patch, wq, tq, radius, eq;
};

// RV_EINVAL with a message for a parameter out of range or a frame of more
// than 2^24 pixels (`what` names the caller in the message).
int dcp_check(const DcpParams& p, int H, int W, const char* what);

// Workspace bytes; the arguments are already checked.
size_t dcp_ws_bytes(int B, int H, int W, int radius);

// in -> out.  flags: nullptr, or the chain gate's per-frame flags (frames it
// passed through are skipped).  air_out, t_out: nullable.
void launch_dcp(const uint8_t* in, uint8_t* out, int B, int H, int W, int pitch,
                const DcpParams& p, void* ws, int32_t* air_out, uint8_t* t_out, const int* flags,
                hipStream_t s);

}  // namespace rv
