// The sweep handle and the one collective step that the callers outside sweep.hip use (moe_host.hip).
#pragma once
#include <mutex>
#include <string>
#include <vector>
#include <rccl/rccl.h>

#include "gp_handle.h"

struct SweepCounters;  // sweep.hip: the node-wide counters and the host transport's slabs

struct egx_sweep {
    egx_gp *gp = nullptr;
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;
    hipStream_t stream = nullptr;
    // staging of the all-gather, allocated once: kChunk doubles per rank
    static constexpr int64_t kChunk = 262144;  // 2 MiB per rank: a 100 000-point mean + variance pair goes in one piece
    egx::DevMem<double> d_send, d_recv;
    egx::PinMem<double> h_send, h_recv;
    std::mutex mu;
    int64_t n_allgathers = 0;
    // dynamic assignment
    int dynamic = 0;
    SweepCounters *counters = nullptr;  // shared memory (world > 1) or heap (world == 1)
    bool counters_shared = false;
    bool shm_transport = false;  // the all-gather goes through `counters->gather` instead of RCCL (test transport)
    int64_t shm_generation = 0;
    std::string shm_name;
    int64_t call_seq = 0;
    // balance of the last call
    std::vector<int64_t> last_per_rank;
    double last_eval_s = 0.0;
    double timeout_s = 1800.0;
};

namespace egx {
// The exchange of payloads that carry a status word in front (sweep_shard.h: sweep_status_word): all (world x part.size())
// <- every rank's part, ALWAYS reached, whatever local_rc says.  Returns the local error first (with the collective's appended
// to its message if that failed too), then the collective's, then EGX_ERR_PEER "<who>: rank r failed with egx_rc c" for the
// lowest rank whose word is set.  Takes no lock: the caller holds sw->mu and has selected the device.  sw == NULL is a world
// of one without a collective: `all` takes part's storage.
int sweep_exchange_status(egx_sweep *sw, const char *who, int local_rc, const std::string &local_msg, std::vector<double> &part,
                          std::vector<double> &all);
}  // namespace egx
