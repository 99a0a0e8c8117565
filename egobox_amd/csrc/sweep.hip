// Multi-GPU theta sweep behind the C ABI (include/egx_gp.h, egx_sweep_*): one process per GPU; candidate c goes to
// rank c mod world (static) or to whichever rank pulls it first from a node-wide counter in POSIX shared memory
// (dynamic: candidates that are not positive definite return ~10x sooner than the others); every rank evaluates its
// share on its own device through the handle's batched likelihood path, ONE RCCL all-gather of {likelihood, status}
// (16 B per candidate and rank) over xGMI assembles the result on every rank.
//
// Failure safety: the all-gather is ALWAYS reached.  A rank whose local work failed contributes a poisoned payload
// (sweep_shard.h) and returns its error afterwards; the other ranks return EGX_ERR_PEER with the failed rank in the
// message.  The staging buffers are allocated once in egx_sweep_create (payloads larger than them go in chunks), and
// the wait for the collective has a deadline (EGX_SWEEP_TIMEOUT_S, default 1800 s) after which the communicator is
// aborted instead of blocking for ever on a peer that died.
//
// Reference seam: the rayon multistart of crates/gp/src/algorithm.rs:928-945 (independent likelihood evaluations,
// arg-min reduce :942-945).  Evaluations at different theta share nothing but the replicated (4 MiB) training set, so
// there is no data-path collective besides this gather.
//
// RCCL is bound at run time (dlopen of librccl.so.1 on the first sweep call): libegx_gp_hip.so itself keeps
// libamdhip64 as its only link-time dependency, and single-GPU users never load the collective library.
#include "gp_handle.h"
#include "sweep_internal.h"
#include "sweep_shard.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <cstdio>
#include <rccl/rccl.h>

namespace egx {

struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;  // optional
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    std::string err;
};

static RcclApi &rccl() {
    static RcclApi api = [] {
        RcclApi a;
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *nm : names) {
            a.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
            if (a.lib) break;
        }
        if (!a.lib) {
            const char *e = dlerror();
            a.err = std::string("cannot load librccl.so.1: ") + (e ? e : "unknown error");
            return a;
        }
#define EGX_SYM(field, name)                                                  \
    a.field = reinterpret_cast<decltype(a.field)>(dlsym(a.lib, name));        \
    if (!a.field && a.err.empty()) a.err = std::string("librccl: missing symbol ") + name;
        EGX_SYM(GetUniqueId, "ncclGetUniqueId");
        EGX_SYM(CommInitRank, "ncclCommInitRank");
        EGX_SYM(CommDestroy, "ncclCommDestroy");
        EGX_SYM(AllGather, "ncclAllGather");
        EGX_SYM(GetErrorString, "ncclGetErrorString");
        EGX_SYM(GetVersion, "ncclGetVersion");
#undef EGX_SYM
        a.CommAbort = reinterpret_cast<decltype(a.CommAbort)>(dlsym(a.lib, "ncclCommAbort"));
        return a;
    }();
    return api;
}

#define EGX_NCCL_CHECK(expr)                                                                   \
    do {                                                                                       \
        ncclResult_t _r = (expr);                                                              \
        if (_r != ncclSuccess) {                                                               \
            ::egx::set_error(std::string(#expr) + ": " + ::egx::rccl().GetErrorString(_r));    \
            return EGX_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

}  // namespace egx

using namespace egx;

// node-wide candidate counters of the dynamic assignment: call number s of a sweep uses slot s % kSlots; rank 0 zeroes
// slot (s + kSlots / 2) % kSlots at the start of call s (nobody touches that slot for the next kSlots / 2 - 1 calls, and
// every call ends with an all-gather, which no rank leaves before every rank has stopped pulling)
struct SweepCounters {
    static constexpr int kSlots = 64;
    std::atomic<int64_t> next[kSlots];
    // HOST TRANSPORT of the all-gather (EGX_SWEEP_TRANSPORT=shm, see egx_sweep_create): two monotonic arrival counters
    // (a barrier = "add one, wait until the count reaches generation x world") and one slab per rank
    static constexpr int kMaxWorld = 16;
    static constexpr int64_t kSlab = 8192;  // doubles per rank and round
    std::atomic<int64_t> arrived_a, arrived_b;
    double gather[kMaxWorld * kSlab];
};
static_assert(std::atomic<int64_t>::is_always_lock_free, "the shared counters must be plain lock-free words");


namespace {

// candidates of one rank in the order it evaluates them
struct StaticSource final : egx::CandidateSource {
    int64_t k, next;
    int world;
    StaticSource(int64_t k_, int rank, int world_) : k(k_), next(rank), world(world_) {}
    int pull(int want, int64_t *out) override {
        int got = 0;
        while (got < want && next < k) {
            out[got++] = next;
            next += world;
        }
        return got;
    }
};
struct DynamicSource final : egx::CandidateSource {
    std::atomic<int64_t> *ctr;
    int64_t k;
    DynamicSource(std::atomic<int64_t> *c, int64_t k_) : ctr(c), k(k_) {}
    int pull(int want, int64_t *out) override {
        if (ctr->load(std::memory_order_relaxed) >= k) return 0;
        const int64_t c0 = ctr->fetch_add(want, std::memory_order_relaxed);
        int got = 0;
        for (int64_t c = c0; c < c0 + want && c < k; c++) out[got++] = c;
        return got;
    }
};

// wait for the sweep's stream with a deadline; on expiry the communicator is aborted (a peer died or never arrived)
int sweep_wait(egx_sweep *sw) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0;; spins++) {
        const hipError_t q = hipStreamQuery(sw->stream);
        if (q == hipSuccess) return EGX_SUCCESS;
        if (q != hipErrorNotReady) {
            set_error(std::string("sweep collective: ") + hipGetErrorString(q));
            (void)hipGetLastError();
            return EGX_ERR_HIP;
        }
        if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if ((spins & 1023) == 1023) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (el > sw->timeout_s) {
                if (sw->comm && rccl().CommAbort) {
                    rccl().CommAbort(sw->comm);
                    sw->comm = nullptr;
                }
                set_error("sweep collective: no answer from the other ranks within " + std::to_string((int)sw->timeout_s) +
                          " s (EGX_SWEEP_TIMEOUT_S); communicator aborted");
                return EGX_ERR_PEER;
            }
        }
    }
}

}  // namespace

// The HOST transport (EGX_SWEEP_TRANSPORT=shm): the same all-gather through the ranks' shared-memory segment.  It
// exists so that the world > 1 logic of this file -- sharding, the dynamic counter, poisoned payloads, the deadline --
// can EXECUTE where RCCL cannot build a communicator: several ranks on ONE GPU (RCCL refuses duplicate devices), i.e. the
// one-GPU box the test-suite runs on (tests/test_gpu_configs.py::test_sweep_two_ranks_*).  The payload is 16 bytes per
// candidate either way; the product transport is RCCL (ncclAllGather over xGMI), which every run with a communicator uses.
static int shm_barrier(egx_sweep *sw, std::atomic<int64_t> &ctr, int64_t generation) {
    ctr.fetch_add(1, std::memory_order_acq_rel);
    const int64_t want = generation * sw->world;
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t spins = 0; ctr.load(std::memory_order_acquire) < want; spins++) {
        if (spins > 4000) std::this_thread::sleep_for(std::chrono::microseconds(20));
        if ((spins & 4095) == 4095 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > sw->timeout_s) {
            set_error("sweep collective (host transport): no answer from the other ranks within " +
                      std::to_string((int)sw->timeout_s) + " s (EGX_SWEEP_TIMEOUT_S)");
            return EGX_ERR_PEER;
        }
    }
    return EGX_SUCCESS;
}
static int shm_allgather_doubles(egx_sweep *sw, const double *send, int64_t count, double *recv) {
    SweepCounters *sc = sw->counters;
    for (int64_t off = 0; off < count; off += SweepCounters::kSlab) {
        const int64_t len = std::min<int64_t>(SweepCounters::kSlab, count - off);
        const int64_t gen = ++sw->shm_generation;
        std::memcpy(sc->gather + (size_t)sw->rank * SweepCounters::kSlab, send + off, sizeof(double) * len);
        EGX_RC(shm_barrier(sw, sc->arrived_a, gen));  // every slab of this round is written
        for (int r = 0; r < sw->world; r++)
            std::memcpy(recv + (size_t)r * count + off, sc->gather + (size_t)r * SweepCounters::kSlab, sizeof(double) * len);
        EGX_RC(shm_barrier(sw, sc->arrived_b, gen));  // ... and read by everybody before the next round overwrites it
        sw->n_allgathers++;
    }
    return EGX_SUCCESS;
}

// all ranks: recv (world x count doubles) <- concatenation over ranks of send (count doubles); host buffers, pinned
// staging allocated in egx_sweep_create, one ncclAllGather per kChunk doubles on the sweep's stream
static int sweep_allgather_doubles(egx_sweep *sw, const double *send, int64_t count, double *recv) {
    if (sw->world == 1 && !sw->comm) {
        std::memcpy(recv, send, sizeof(double) * count);
        return EGX_SUCCESS;
    }
    if (sw->shm_transport) return shm_allgather_doubles(sw, send, count, recv);
    if (!sw->comm) {
        set_error("sweep collective: the communicator was aborted by an earlier failure");
        return EGX_ERR_PEER;
    }
    for (int64_t off = 0; off < count; off += egx_sweep::kChunk) {
        const int64_t len = std::min<int64_t>(egx_sweep::kChunk, count - off);
        std::memcpy(sw->h_send, send + off, sizeof(double) * len);
        EGX_HIP_CHECK(hipMemcpyAsync(sw->d_send, sw->h_send, sizeof(double) * len, hipMemcpyHostToDevice, sw->stream));
        EGX_NCCL_CHECK(rccl().AllGather(sw->d_send, sw->d_recv, (size_t)len, ncclDouble, sw->comm, sw->stream));
        EGX_HIP_CHECK(hipMemcpyAsync(sw->h_recv, sw->d_recv, sizeof(double) * len * sw->world, hipMemcpyDeviceToHost,
                                     sw->stream));
        EGX_RC(sweep_wait(sw));
        for (int r = 0; r < sw->world; r++)
            std::memcpy(recv + (size_t)r * count + off, sw->h_recv + (size_t)r * len, sizeof(double) * len);
        sw->n_allgathers++;
    }
    return EGX_SUCCESS;
}

int egx::sweep_exchange_status(egx_sweep *sw, const char *who, int local_rc, const std::string &local_msg, std::vector<double> &part,
                               std::vector<double> &all) {
    const int world = sw ? sw->world : 1;
    if (sw) {
        all.resize(part.size() * (size_t)world);
        const int coll_rc = sweep_allgather_doubles(sw, part.data(), (int64_t)part.size(), all.data());
        if (coll_rc) {
            if (local_rc) set_error(local_msg + " (and the collective failed: " + last_error_string() + ")");
            return local_rc ? local_rc : coll_rc;
        }
    } else {
        all.swap(part);
    }
    if (local_rc) {
        set_error(local_msg);
        return local_rc;
    }
    const SweepFailure f = sweep_first_failure(all.data(), world, all.size() / (size_t)world);
    if (f.rank >= 0) {
        set_error(std::string(who) + ": rank " + std::to_string(f.rank) + " failed with egx_rc " + std::to_string(f.rc));
        return EGX_ERR_PEER;
    }
    return EGX_SUCCESS;
}


extern "C" {

int32_t egx_sweep_unique_id(void *id_out) {
    if (!id_out) {
        set_error("egx_sweep_unique_id: NULL output");
        return EGX_ERR_INVALID_VALUE;
    }
    static_assert(sizeof(ncclUniqueId) == EGX_SWEEP_ID_BYTES, "EGX_SWEEP_ID_BYTES must match ncclUniqueId");
    RcclApi &api = rccl();
    if (!api.err.empty()) {
        set_error(api.err);
        return EGX_ERR_UNSUPPORTED;
    }
    ncclUniqueId id;
    EGX_NCCL_CHECK(api.GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof id);
    return EGX_SUCCESS;
}

int32_t egx_sweep_create(const egx_gp_config *cfg_in, const double *x, const double *y, int64_t n, int64_t d,
                         const void *nccl_id, int32_t rank, int32_t world, egx_sweep **out) {
    if (!out) {
        set_error("out handle pointer is NULL");
        return EGX_ERR_INVALID_VALUE;
    }
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) {
        set_error("egx_sweep_create: need 0 <= rank < world, got rank " + std::to_string(rank) + " world " +
                  std::to_string(world));
        return EGX_ERR_INVALID_VALUE;
    }
    if (world > 1 && !nccl_id) {
        set_error("egx_sweep_create: world > 1 needs the unique id of egx_sweep_unique_id (from rank 0)");
        return EGX_ERR_INVALID_VALUE;
    }
    egx_gp_config cfg;
    if (cfg_in) cfg = *cfg_in; else egx_gp_config_default(&cfg);
    if (cfg.n_workspaces < 2) cfg.n_workspaces = 2;  // two candidates in flight per GPU (panel latency hidden)
    egx_sweep *sw = new egx_sweep();
    sw->rank = rank;
    sw->world = world;
    if (const char *e = std::getenv("EGX_SWEEP_TIMEOUT_S")) {
        const double t = std::atof(e);
        if (t > 0.0) sw->timeout_s = t;
    }
    int rc = egx_gp_create(&cfg, x, y, n, d, &sw->gp);
    if (rc) {
        delete sw;
        return rc;
    }
    auto fail = [&](int r) {
        egx_sweep_destroy(sw);
        return r;
    };
    if (hipSetDevice(sw->gp->device) != hipSuccess ||
        hipStreamCreateWithFlags(&sw->stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("egx_sweep_create: stream creation failed");
        (void)hipGetLastError();
        return fail(EGX_ERR_HIP);
    }
    {   // staging of the collective: allocated here, never inside a collective call
        const size_t one = (size_t)egx_sweep::kChunk;
        if (sw->d_send.alloc(one) || sw->d_recv.alloc(one * world) || sw->h_send.alloc(one) || sw->h_recv.alloc(one * world)) {
            set_error("egx_sweep_create: staging buffers");
            return fail(EGX_ERR_HIP);
        }
    }
    // candidate counters of the dynamic assignment: shared by the ranks of this node (named after the unique id)
    if (world > 1) {
        uint64_t hsh = 1469598103934665603ull;  // FNV-1a of the id
        for (int i = 0; i < EGX_SWEEP_ID_BYTES; i++) hsh = (hsh ^ ((const unsigned char *)nccl_id)[i]) * 1099511628211ull;
        char nm[64];
        std::snprintf(nm, sizeof nm, "/egx_sweep_%016llx", (unsigned long long)hsh);
        sw->shm_name = nm;
        const int fd = shm_open(nm, O_CREAT | O_RDWR, 0600);
        void *mem = MAP_FAILED;
        if (fd >= 0 && ftruncate(fd, sizeof(SweepCounters)) == 0)  // a new object is zero filled
            mem = mmap(nullptr, sizeof(SweepCounters), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        if (fd >= 0) close(fd);
        if (mem != MAP_FAILED) {
            sw->counters = static_cast<SweepCounters *>(mem);
            sw->counters_shared = true;
        }  // else: only the static assignment is available (egx_sweep_set_assignment reports it)
    } else {
        sw->counters = new SweepCounters();
        for (auto &c : sw->counters->next) c.store(0);
    }
    {
        const char *tr = std::getenv("EGX_SWEEP_TRANSPORT");
        if (tr && std::string(tr) == "shm" && world > 1) {
            if (!sw->counters_shared || world > SweepCounters::kMaxWorld) {
                set_error("egx_sweep_create: the host transport needs the shared-memory segment and world <= 16");
                return fail(EGX_ERR_UNSUPPORTED);
            }
            sw->shm_transport = true;
        }
    }
    if (nccl_id && !sw->shm_transport) {
        RcclApi &api = rccl();
        if (!api.err.empty()) {
            set_error(api.err);
            return fail(EGX_ERR_UNSUPPORTED);
        }
        ncclUniqueId id;
        std::memcpy(&id, nccl_id, sizeof id);
        // RCCL >= 2.26 prints a version banner to STDOUT on the first communicator: keep the host's stdout clean (it
        // may carry a protocol, e.g. bench.py's single JSON line) by pointing fd 1 at stderr for the duration of the
        // init.  EGX_RCCL_BANNER=1 leaves it alone.
        const char *keep = std::getenv("EGX_RCCL_BANNER");
        int saved = -1;
        if (!(keep && keep[0] == '1')) {
            fflush(stdout);
            saved = dup(1);
            if (saved >= 0) dup2(2, 1);
        }
        ncclResult_t r = api.CommInitRank(&sw->comm, world, id, rank);
        if (saved >= 0) {
            fflush(stdout);
            dup2(saved, 1);
            close(saved);
        }
        if (r != ncclSuccess) {
            set_error(std::string("ncclCommInitRank: ") + api.GetErrorString(r));
            sw->comm = nullptr;
            return fail(EGX_ERR_HIP);
        }
    }
    *out = sw;
    return EGX_SUCCESS;
}

void egx_sweep_destroy(egx_sweep *sw) {
    if (!sw) return;
    if (sw->gp) hipSetDevice(sw->gp->device);
    if (sw->comm) rccl().CommDestroy(sw->comm);
    if (sw->stream) hipStreamDestroy(sw->stream);
    if (sw->counters) {
        if (sw->counters_shared) {
            munmap(sw->counters, sizeof(SweepCounters));
            if (sw->rank == 0) shm_unlink(sw->shm_name.c_str());
        } else {
            delete sw->counters;
        }
    }
    if (sw->gp) egx_gp_destroy(sw->gp);
    delete sw;
}

egx_gp *egx_sweep_handle(egx_sweep *sw) { return sw ? sw->gp : nullptr; }

int32_t egx_sweep_info(const egx_sweep *sw, int32_t *rank, int32_t *world, int32_t *rccl_ranks, int32_t *rccl_version,
                       int64_t *n_allgathers) {
    if (!sw) {
        set_error("NULL sweep handle");
        return EGX_ERR_INVALID_VALUE;
    }
    if (rank) *rank = sw->rank;
    if (world) *world = sw->world;
    if (rccl_ranks) *rccl_ranks = sw->comm ? sw->world : 0;
    if (rccl_version) {
        int v = 0;
        if (sw->comm && rccl().GetVersion) rccl().GetVersion(&v);
        *rccl_version = v;
    }
    if (n_allgathers) *n_allgathers = sw->n_allgathers;
    return EGX_SUCCESS;
}

int32_t egx_sweep_set_assignment(egx_sweep *sw, int32_t dynamic) {
    if (!sw) {
        set_error("NULL sweep handle");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(sw->mu);
    if (dynamic && !sw->counters) {
        set_error("egx_sweep_set_assignment: no shared-memory counters on this node (shm_open failed): static only");
        return EGX_ERR_UNSUPPORTED;
    }
    sw->dynamic = dynamic ? 1 : 0;
    return EGX_SUCCESS;
}

int32_t egx_sweep_last_balance(const egx_sweep *sw, int64_t *per_rank, double *local_eval_s) {
    if (!sw) {
        set_error("NULL sweep handle");
        return EGX_ERR_INVALID_VALUE;
    }
    if (per_rank)
        for (int r = 0; r < sw->world; r++) per_rank[r] = r < (int)sw->last_per_rank.size() ? sw->last_per_rank[r] : 0;
    if (local_eval_s) *local_eval_s = sw->last_eval_s;
    return EGX_SUCCESS;
}

int32_t egx_sweep_likelihood(egx_sweep *sw, const double *thetas, int64_t k, int64_t theta_len, double *lkh,
                             int32_t *status) {
    if (!sw || k < 0 || (k > 0 && (!thetas || !lkh || !status)) || theta_len < 1) {
        set_error("egx_sweep_likelihood: NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(sw->mu);
    if (k == 0) return EGX_SUCCESS;
    const int world = sw->world, rank = sw->rank;
    // ---- local part: every failure from here on is CARRIED to the collective, never returned before it
    int local_rc = EGX_SUCCESS;
    std::string local_msg;
    std::vector<double> lk(k);
    std::vector<int32_t> st(k);
    std::vector<char> mine(k, 0);
    const int64_t seq = sw->call_seq++;
    const auto t0 = std::chrono::steady_clock::now();
    {
        std::atomic<int64_t> *ctr = nullptr;
        // The slot of call `seq` was zeroed by rank 0 half a ring earlier, when every rank had long left the slot's previous
        // use (the all-gather of each call is a barrier).  The sequence number advances on EVERY call, so the look-ahead slot
        // is recycled on every call too -- static ones included: a slot dirtied by a dynamic call must be clean again 64
        // calls later whatever mode the call half a ring in between was in.
        if (sw->counters && rank == 0)
            sw->counters->next[(seq + SweepCounters::kSlots / 2) % SweepCounters::kSlots].store(0);
        if (sw->dynamic && sw->counters) ctr = &sw->counters->next[seq % SweepCounters::kSlots];
        StaticSource ssrc(k, rank, world);
        DynamicSource dsrc(ctr, k);
        egx::CandidateSource *src = ctr ? static_cast<egx::CandidateSource *>(&dsrc) : &ssrc;
        local_rc = set_device(sw->gp);
        if (!local_rc) {
            std::unique_lock<std::shared_mutex> glock(sw->gp->mu);
            local_rc = likelihood_batch_core(sw->gp, thetas, k, theta_len, lk.data(), st.data(), src, mine.data());
        }
        if (local_rc) local_msg = last_error_string();
    }
    sw->last_eval_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::vector<double> send;
    if (local_rc) {
        send = sweep_poison(k, local_rc);
    } else {
        send = sweep_payload(k);
        for (int64_t c = 0; c < k; c++)
            if (mine[c]) sweep_put(send, c, lk[c], st[c]);
    }
    // ---- the collective
    std::vector<double> recv((size_t)k * 2 * world);
    const int coll_rc = sweep_allgather_doubles(sw, send.data(), k * 2, recv.data());
    if (coll_rc) {
        if (local_rc) set_error(local_msg + " (and the collective failed: " + last_error_string() + ")");
        return local_rc ? local_rc : coll_rc;
    }
    const SweepVerdict v = sweep_unpack(recv.data(), k, world, lkh, status, EGX_STATUS_RANK_FAILED);
    sw->last_per_rank = v.per_rank;
    if (local_rc) {
        set_error(local_msg);
        return local_rc;
    }
    if (v.failed_rank >= 0) {
        set_error("egx_sweep_likelihood: rank " + std::to_string(v.failed_rank) + " failed with egx_rc " +
                  std::to_string(v.failed_rc) + "; " + std::to_string(v.missing) + " of " + std::to_string(k) +
                  " candidates have no result (status EGX_STATUS_RANK_FAILED)");
        return EGX_ERR_PEER;
    }
    if (v.missing || v.duplicate) {
        set_error("egx_sweep_likelihood: assignment inconsistent across ranks (" + std::to_string(v.missing) + " missing, " +
                  std::to_string(v.duplicate) + " duplicated): did every rank select the same assignment mode?");
        return EGX_ERR_PEER;
    }
    return EGX_SUCCESS;
}

int32_t egx_sweep_allgather(egx_sweep *sw, const double *send, int64_t count, double *recv) {
    if (!sw || count < 0 || (count > 0 && (!send || !recv))) {
        set_error("egx_sweep_allgather: NULL argument");
        return EGX_ERR_INVALID_VALUE;
    }
    std::lock_guard<std::mutex> lock(sw->mu);
    if (count == 0) return EGX_SUCCESS;
    // (a failing set_device is carried into the collective as NaNs: every rank still arrives)
    const int dev_rc = set_device(sw->gp);
    const std::string dev_msg = dev_rc ? last_error_string() : std::string();
    std::vector<double> poisoned;
    if (dev_rc) poisoned.assign((size_t)count, std::numeric_limits<double>::quiet_NaN());
    const int rc = sweep_allgather_doubles(sw, dev_rc ? poisoned.data() : send, count, recv);
    if (dev_rc) {
        set_error(dev_msg);
        return dev_rc;
    }
    return rc;
}


// ---- tuned fit over the ranks of a sweep (SURVEY 8e x 8f rank 2) --------------------------------------------------
// GpValidParams::fit with ThetaTuning::Full (crates/gp/src/algorithm.rs:873-960): the reference runs its n_start + 1 COBYLA
// runs as rayon tasks on one host (:928-945).  Here start s belongs to rank s mod world; a rank advances the machines of
// its starts in lock-step on its own GPU (fit_run_starts), ONE all-gather carries every start's (objective, evaluations,
// minimiser) to every rank, all ranks reduce in start order (first minimum wins, :942-945) and factor the winner on their
// replica.  An evaluation returns the same bits wherever and in whichever batch it runs, so every start walks the trajectory
// it walks on one GPU and the fitted model is bit for bit the one egx_gp_fit returns.
int32_t egx_sweep_fit(egx_sweep *sw, const double *theta0s, int64_t n_starts, const double *lo, const double *hi,
                      int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out) {
    if (!sw || !theta0s || !lo || !hi || n_starts < 1) {
        set_error("egx_sweep_fit: NULL argument / no start point");
        return EGX_ERR_INVALID_VALUE;
    }
    egx_gp *gp = sw->gp;
    const int h = gp->h, world = sw->world;
    const std::vector<int> active = fit::all_active(h);
    std::vector<StartResult> results;
    // one critical section on the replica from the first evaluation to the finalized model (the all-gather included: it has
    // its own deadline), as egx_gp_fit is on a plain handle.  Lock order as in egx_sweep_likelihood: the sweep, then its model.
    std::lock_guard<std::mutex> lock(sw->mu);
    std::unique_lock<std::shared_mutex> glock(gp->mu);
    int local_rc = fit_run_starts(gp, theta0s, active, theta0s, n_starts, lo, hi, bounds_len, max_eval, sw->rank, world, results);
    const std::string local_msg = local_rc ? last_error_string() : std::string();
    // payload: [status | per start: objective, evaluations, minimiser (h)], NaN objective for the starts of other ranks
    const size_t per = (size_t)h + 2;
    std::vector<double> part(1 + (size_t)n_starts * per, std::numeric_limits<double>::quiet_NaN());
    part[0] = sweep_status_word(local_rc);
    if (!local_rc)
        for (int64_t s = sw->rank; s < n_starts; s += world) {
            double *q = part.data() + 1 + (size_t)s * per;
            q[0] = results[(size_t)s].f;
            q[1] = (double)results[(size_t)s].evals;
            for (int i = 0; i < h; i++) q[2 + i] = results[(size_t)s].x[(size_t)i];
        }
    std::vector<double> all;
    (void)set_device(gp);
    EGX_RC(sweep_exchange_status(sw, "egx_sweep_fit", local_rc, local_msg, part, all));
    results.clear();
    for (int64_t s = 0; s < n_starts; s++) {
        const double *q = all.data() + (size_t)(s % world) * part.size() + 1 + (size_t)s * per;
        results.push_back(StartResult{q[0], std::vector<double>(q + 2, q + 2 + h), (int64_t)q[1]});
    }
    return fit_reduce_finalize(gp, theta0s, active, theta0s, results, n_evals_out);
}

}  // extern "C"
