// Launch interface of gba_kernels.hip (Optimizer::GlobalBundleAdjustemnt: one large problem spread over the device),
// used by the msf_global_bundle_adjust* entry points in msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gba_solve.h"

namespace msf {

// One call: the problem, the schedule, the scratch (gba::layout placed on device memory), where the results go
// (device pointers, one problem of msf_ba_result) and the device stop word (null: none).
struct GbaCall {
  ba::Problem p;
  ba::Params prm;
  gba::Scratch s;
  ba::Out out;
  const int32_t* d_stop;
};

// The checking launch: every edge index and the order of edge_point, the free cameras, the stop word.  Reads nothing
// through an index.  Needs s.rec only.  Waits for the stream; *verdict is the record the host reads (pinned memory).
hipError_t gba_check(const GbaCall& call, gba::Record* verdict, hipStream_t st);

// The whole schedule on a problem that gba_check passed with n_free free cameras, s.w laid out for them; `pinned`: the
// record the host reads after every wait (s.rec is cleared first: it need not be the block gba_check wrote); host_stop: null or a host word another thread may set.  Returns when the
// problem is finished (the stream is idle); *status = the rounds run, written to out.status as well.
hipError_t gba_solve(const GbaCall& call, int n_free, int32_t stop_at_entry, gba::Record* pinned,
                     const volatile int32_t* host_stop, hipStream_t st, int* status);

// out.status = -1 and nothing else
hipError_t gba_refuse(const GbaCall& call, hipStream_t st);

}  // namespace msf
