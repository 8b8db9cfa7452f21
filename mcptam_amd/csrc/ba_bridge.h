// ba_bridge.h -- what the image-path unit (img_api.hip) may ask of a solver handle (ba_solver.hip) without seeing struct mcp_ba:
// the device pointers of the CURRENT state, the stream they are written on, and the id -> index tables.  Internal: not part of
// include/mcp_ba.h, nothing here is exported with C linkage.  Used by mcp_ba_write_back (include/mcp_img.h).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mcp_ba.h"

namespace mcp {

struct BaDeviceState {
  int device;                 // HIP device ordinal of the handle
  hipStream_t stream;         // the solver's main stream: everything that wrote pose / point is ordered on it
  const double* pose;         // npose x 12 (R row-major 9, t 3), add order, current state
  const double* point;        // npoint x 3, add order, current state (a point in its own chain's frame; a fixed point in the world frame)
  int npose, npoint;
};
// 0 and *out filled; -1 + mcp_last_error(): the handle was never prepared (or was changed since), or it is a sharded (multi-rank) handle
// -- an all-reduce hook or a communicator is installed.  `who` prefixes the message.
int ba_bridge_state(mcp_ba* h, const char* who, BaDeviceState* out);
// point `id`: its index in BaDeviceState::point, the fixed flag and the solver's number of its own chain; -1: `id` is not a point
int ba_bridge_point(const mcp_ba* h, int id, int* index, int* fixed, int* chain);
// the solver's chains: how many, and chain c as pose INDICES into BaDeviceState::pose (v[0 .. len))
int ba_bridge_num_chains(const mcp_ba* h);
void ba_bridge_chain(const mcp_ba* h, int c, int* len, int v[MCP_MAX_CHAIN]);
// a chain given as pose ids (as mcp_ba_add_meas takes them): the solver's number of it (>= 0); -1: well-formed but no point or measurement
// of the bundle uses it (v receives its pose indices); -2: malformed (n < 1, n > MCP_MAX_CHAIN, or an entry that is not a pose)
int ba_bridge_lookup_chain(const mcp_ba* h, const int* ids, int n, int v[MCP_MAX_CHAIN]);

}  // namespace mcp
