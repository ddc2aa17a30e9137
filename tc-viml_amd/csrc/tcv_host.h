// Host-side data model behind the C-ABI of include/tcv.h: the ceres::Problem-shaped graph
// (reference vins_estimator/src/estimator.cpp:1679-1886), the MarginalizationInfo-shaped prior
// (factor/marginalization_factor.h:46-72) and the packer that turns a problem into the
// device-resident plan + data of tcv_packed.h; behind the batch (tcv_batch.h, included at the end), what the side tables beside its
// plans share (PlanTable, BlockMap) and the covariance's table builders.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tcv.h"
#include "tcv_packed.h"
#include "tcv_hostpool.h"
#include "tcv_runtime.h"      // streams, pools, error text, StagedTransfer / RoundTrip

namespace tcv {
// a device allocation shared between its producer (a batch) and the handles that still read it (device-resident priors)
struct DevBlob {
    void *p = nullptr;
    int dev = 0;
    // non-null: recorded behind the commands that fill the blob, by a producer that did not wait for them (tcv_preintegrate_device): a
    // consumer on another stream waits for it (wait_ready), a host reader synchronises it
    hipEvent_t ready = nullptr;
    int wait_ready(hipStream_t consumer) const;      // TCV_OK or TCV_ERR_HIP
    int sync_ready() const;
    ~DevBlob();
};
}  // namespace tcv

struct tcv_prior {
    int m = 0, n = 0;
    std::vector<int> size, idx;       // keep_block_size / keep_block_idx (idx relative to m, i.e. column of J0)
    std::vector<int> xoff;            // offset of every block in x0
    int xsize = 0;                    // doubles of x0 (= keep_block_data, concatenated), whether or not it is on the host
    mutable std::vector<double> x0;   // keep_block_data, concatenated
    mutable std::vector<double> J0, r0;   // linearized_jacobians (n x n column-major), linearized_residuals
    std::vector<double *> addr;       // addresses of the kept blocks at marginalisation time (un-shifted)
    std::vector<double> As, bs;       // Schur system A', b' the factors were taken from (parity/debug, may be empty)
    // device-resident form (tcv_batch_get_priors_device): J0 | r0 | the marginalisation problem's state vector stay in the producing
    // batch's result buffer; `host` says whether x0 / J0 / r0 above have been materialised (tcv_prior_host)
    std::shared_ptr<tcv::DevBlob> dev;
    const double *d_block = nullptr;  // this window's result block in that buffer (layout: tcv_marg.h MARG_OUT_*)
    int k0 = 0;                       // leading rows of J0 | r0 that are exact zeros (tcv_packed.h prior_zero_rows, computed on the device)
                                      // -1: not known on the host (tcv_batch_get_priors_device_async: the marginalisation may still be running) --
    const int *d_k0 = nullptr;        //     the consumer reads it on the device, behind the producer's event (dev->ready): [status | k0] of this window
    const int *d_status = nullptr;
    std::vector<int> x_goff;          // per kept block: offset of its values in the result block's state region
    mutable bool host = true;
    mutable std::mutex mu;            // materialisation (several packing threads may ask for it at once)
};
// IntegrationBase on the device (tcv_preintegrate_device): the kernel's output record [delta_p 3 | delta_q 4 | delta_v 3 | ba 3 | bg 3 |
// sum_dt | jacobian 225 | covariance 225] stays in HBM
struct tcv_preint {
    std::shared_ptr<tcv::DevBlob> dev;
    const double *d_out = nullptr;
    double sum_dt = 0.0;
    mutable bool host = false;
    mutable tcv_imu_preintegration pod;
    mutable std::mutex mu;
};
int tcv_preint_host(const tcv_preint *pre);      // materialises `pod` (once); TCV_OK or an error
// the prior's numbers on the host: no-op for a host prior, one device-to-host copy (once) for a device-resident one; TCV_OK or an error
int tcv_prior_host(const tcv_prior *pr);

namespace tcv {

struct ParamBlock {
    double *addr;
    int size, kind;
    bool constant;
};
struct ImuFac { tcv_imu_preintegration pre; int b[4]; const tcv_preint *dev = nullptr; };   // dev: the constants live on the device, `pre` holds sum_dt only
struct ProjFac { double pts[6]; double sqrt_info, loss_a; int b[4]; double aux[8]; int btd; };   // btd >= 0: ProjectionTdFactor on block btd
struct LineFac { double d[9]; double K[9], R[9], T[3]; double loss_a; int b; };
struct PriorFac { const tcv_prior *prior; std::vector<int> b; };

// allocator of the plans' int pools: blocks of the process-wide free list (tcv_hostpool.h)
template <class T> struct PlanAlloc {
    typedef T value_type;
    PlanAlloc() = default;
    template <class U> PlanAlloc(const PlanAlloc<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(plan_block_alloc(n * sizeof(T))); }
    void deallocate(T *p, size_t n) { plan_block_free(p, n * sizeof(T)); }
    template <class U> bool operator==(const PlanAlloc<U> &) const { return true; }
    template <class U> bool operator!=(const PlanAlloc<U> &) const { return false; }
};
typedef std::vector<int, PlanAlloc<int>> PlanInts;

// structural half of a packed window (plan header + int pool + host-side maps): a function of the graph STRUCTURE only, shared by every
// window with that structure (tcv_pack.cpp keeps a process-wide cache keyed by the structure)
struct PlanTemplate {
    PlanHdr hdr;
    PlanInts ints;
    unsigned long long hash = 0;      // plan_content_hash(hdr, ints), computed once by the packing thread that made the template
    std::vector<int> cam_block, cam_loff, lm_block, proj_order;
};

struct Packed {
    PlanHdr hdr;
    std::shared_ptr<const PlanTemplate> tmpl;   // set when the plan came from / went into the cache: `ints` is then empty and tmpl->ints holds the plan
    PlanInts ints;
    std::vector<double> doubles;
    WinHdr win;
    unsigned long long plan_hash = 0;   // of hdr + plan ints (tcv_batch_create: structure de-duplication without copying 200 KB keys)
    bool key_hashed = false;            // plan_hash was set by the packer from the structure key (a plan built for this window alone: tcv_pack.cpp)
    int dev_imu_doubles = 0;         // > 0: every IMU factor of the window is device-resident: n_imu x 287 doubles in the device-only tail (WinHdr::d_imu points there)
    bool prior_k0_deferred = false;  // the prior's zero-row count is read on the device (tcv_prior::k0 < 0): WinHdr::prior_k0 is patched by the splice kernel
    int batch_dev = -1;              // device the batch is created on (tcv_batch_create; -1: no device-resident input is spliced): a prior / pre-integration
                                     // resident on ANOTHER device goes through the host (peer access is never enabled)
    int dev_prior_doubles = 0;       // > 0: the window's prior is device-resident: doubles of its J0 | r0 | x0 region, which lives in the batch's
                                     // device-only tail (not in the uploaded slice) and is filled by the splice kernel of tcv_batch_create
    // host-side maps for download
    std::vector<int> cam_block;      // problem block index of every camera block
    std::vector<int> cam_loff;       // tangent offset of every camera block (-1 constant)
    std::vector<int> lm_block;       // problem block index of every landmark
    std::vector<int> proj_order;     // sorted position -> original projection factor index
};

}  // namespace tcv

namespace tcv {
// address -> block index of a problem: open addressing in one flat array (a node-based map cost a live estimator 200 small allocations and
// frees per window and frame)
struct AddrIndex {
    std::vector<std::pair<double *, int>> tab;      // power-of-two size; first == nullptr: empty
    size_t used = 0;
    static size_t h(const double *a) { size_t x = (size_t)a >> 3; x *= 0x9E3779B97F4A7C15ull; return x >> 17; }
    int find(double *a) const {
        if (!a || tab.empty()) return -1;      // nullptr marks an empty slot: a NULL key must never match one
        const size_t m = tab.size() - 1;
        for (size_t i = h(a) & m;; i = (i + 1) & m) { if (tab[i].first == a) return tab[i].second; if (!tab[i].first) return -1; }
    }
    void put(double *a, int v) {
        if (!a) return;                          // callers reject NULL addresses before they get here (tcv_problem_add_parameter_block)
        if (2 * (used + 1) > tab.size()) grow();
        const size_t m = tab.size() - 1;
        for (size_t i = h(a) & m;; i = (i + 1) & m) { if (tab[i].first == a) { tab[i].second = v; return; } if (!tab[i].first) { tab[i] = {a, v}; used++; return; } }
    }
    void grow() {
        std::vector<std::pair<double *, int>> old;
        old.swap(tab);
        tab.assign(old.empty() ? 512 : 2 * old.size(), {nullptr, 0});
        used = 0;
        for (auto &kv : old) if (kv.first) put(kv.first, kv.second);
    }
};
}  // namespace tcv

struct tcv_problem {
    std::vector<tcv::ParamBlock> blocks;
    tcv::AddrIndex index;
    std::vector<tcv::ImuFac> imu;
    std::vector<tcv::ProjFac> proj;
    std::vector<tcv::LineFac> line;
    std::vector<tcv::PriorFac> prior;
    double G[3] = {0, 0, 9.8};
    double td_TR = 0.0, td_ROW = 1.0;        // rolling-shutter globals of ProjectionTdFactor
    int line_exact = 0;                      // 1: line factors use the exact derivative of their residual (opt-in extension)
    std::vector<int> frame_pose, frame_sb;   // block ids of para_Pose[i] / para_SpeedBias[i] (gauge fix), may be empty
    // tcv_problem_set_relocalization: block id of relo_Pose (-1: none), relo_frame_local_index, prev_relo_t 3 | prev_relo_r 9
    int relo_block = -1, relo_local = -1;
    double relo_prev[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
};

namespace tcv {
// A side table beside the plans of a batch (the owner lists of the gradient and of S, the landmark slot tables): one device allocation
// [offset of every distinct plan's entry, in ints (long long) | the entries], at least one int behind the offsets.
struct PlanTable { void *d = nullptr; long long *base = nullptr; int *ints = nullptr; };
// entry(w, out) builds the entry of window w's plan (TCV_OK, or a status with the message set); it is asked once per distinct plan, for the
// first window that uses it, in window order.  Allocates, uploads (staged_upload) and frees on failure; the caller frees t->d (dev_free).
int plan_table_create(const tcv_batch *b, const std::function<int(int, std::vector<int> &)> &entry, const char *what_alloc, const char *what_upload, PlanTable *t);
// problem block -> camera block / landmark of the packed window (-1: none) and tangent offset (-1: constant or no camera block)
struct BlockMap {
    const Packed &pk;
    const size_t nb;
    std::vector<int> of;      // [camera block of every problem block | landmark of every problem block]
    BlockMap(const tcv_problem &p, const Packed &packed) : pk(packed), nb(p.blocks.size()), of(2 * nb, -1) {
        for (size_t c = 0; c < pk.cam_block.size(); c++) of[pk.cam_block[c]] = (int)c;
        for (size_t l = 0; l < pk.lm_block.size(); l++) of[nb + pk.lm_block[l]] = (int)l;
    }
    int cam_of(int blk) const { return of[blk]; }
    int lm_of(int blk) const { return of[nb + blk]; }
    int toff(int blk) const { return of[blk] >= 0 ? pk.cam_loff[of[blk]] : -1; }
};
}  // namespace tcv
// The side tables of the marginal covariance (tcv_cov_tables.cpp; layouts: tcv_cov.h): no device call; TCV_OK or a status with the message set
struct tcv_covariance_block;
namespace tcv {
// the problem block of one half of a request and its tangent width (either may be null)
int cov_resolve(const tcv_problem &p, int kind, int index, int *blk, int *width);
// The slots of h_l: per landmark (plan order) the distinct variable blocks of its point factors, in order of first appearance; of a window
// whose owner lists were not refused.
struct CovLmSlots {
    std::vector<int> lmptr{0}, lmfac;           // the point factors (plan order) of landmark l: lmfac[lmptr[l] .. lmptr[l + 1]]
    std::vector<int> sptr{0}, blk, off;         // the slots of landmark l: sptr[l] .. sptr[l + 1]; per slot its problem block and its offset in the J region
    std::vector<std::vector<int>> items;        // per slot its hitem records
    int jdoubles = 0;                           // doubles of the J region, the slots at its end
};
CovLmSlots cov_landmark_slots(const tcv_problem &p, const Packed &pk, const PlanHdr &H);
// the owner lists of S for the plan of a window; refuses (TCV_ERR_UNSUPPORTED) a constant inverse depth and a factor that names one block twice
int cov_owner_lists(const tcv_problem &p, const Packed &pk, const PlanHdr &H, std::vector<int> &out, int *jdoubles);
// the plan's landmark slot table: lsptr, then the slots of every landmark in ascending tangent order
std::vector<int> cov_slot_table(const tcv_problem &p, const Packed &pk, const CovLmSlots &slots);
// the request tables of every window (RQ_*) for a request list, and the sizes of its blocks
int cov_request_tables(const tcv_batch *b, const tcv_covariance_block *blocks, int n_req, std::vector<int> &rq, std::vector<int> &rows, std::vector<int> &cols);
}  // namespace tcv
int tcv_marg_sqrt_source(const tcv_batch *b, int window);   // index of that factor among the solve problem's IMU factors, -1 none
int tcv_marg_attach(tcv_batch *b, tcv_problem *const *marg_problems, double *const *const *marg_drop, const int *marg_num_drop);
int tcv_marg_run(tcv_batch *b, void *stream);
int tcv_marg_get_prior(tcv_batch *b, int window, tcv_prior **out);
void tcv_marg_elapsed(tcv_batch *b);
int tcv_marg_download(tcv_batch *b, int compact);
int tcv_marg_get_priors_device(tcv_batch *b, tcv_prior **out, int n, bool nowait);
int tcv_marg_status_prefetch(tcv_batch *b, void *stream);
bool tcv_marg_has_problem(const tcv_batch *b, int window);      // false: marg_problems[window] was NULL
int tcv_marg_layout_n(const tcv_batch *b, int window);          // n of the prior this window's marginalisation makes (known from the attached problem, before the kernel runs); -1: none
// host only (tcv_problem_marg_plan): one window through the marginalisation packer -- ints = [MargHdr as ints | int pool], doubles = the
// double pool; both empty when the marginalisation keeps nothing
int tcv_marg_plan(const tcv_problem &p, double *const *drop, int ndrop, const tcv_problem *solve_p, const tcv::Packed *solve_pk,
                  std::vector<int> &ints, std::vector<double> &doubles);
// copies device-resident priors into a batch's data pool (one job per window that holds one): launched by tcv_batch_create on the stream
// of its upload, behind it
namespace tcv {
// kind 0: a prior (src = the result block of its window, tcv_marg.h MARG_OUT_*); kind 1: an IMU factor's constants (src = the
// pre-integration kernel's output record; n, k0, nblk unused)
struct PriorSplice {
    const double *src; long long dst; int n, k0, nblk, kind; int goff[32], size[32];
    const int *k0_src;      // non-null: k0 is read here, on the device ([status | k0] of the producing marginalisation), and written to the window header `win`
    int win, pad;
};
enum { PRIOR_SPLICE_MAX_BLOCKS = 32 };
int launch_prior_splice(const PriorSplice *d_jobs, int njobs, double *d_dpool, void *d_win_headers, hipStream_t st);
}  // namespace tcv

namespace tcv {
int solver_variant();      // tcv_set_solver_variant (tcv_batch_create.cpp): 0 chain layout when the graph allows it, 1 always the dense 171-dim layout
// returns TCV_OK or a negative status; fills out.  imu_sqrt: optional host-provided sqrt_info (n_imu x 225).
// mode: 0 = chain layout when the graph allows it (speed-bias blocks form chains), else dense; 1 = dense layout
// chain_lds: LDS doubles of a chain-layout workgroup (0: chain_lds_doubles(), half a CU's LDS so that two workgroups share a CU)
// plan_only: plan + the size of the data half (out.win.n_doubles); the data is then written by pack_problem_data into a buffer of the
// caller (one upload buffer per batch)
// coop_chunks > 0: plan for the cooperative (small-batch) kernel with at least that many visual chunks (tcv_packed.h COOP_*)
int pack_problem(const tcv_problem &p, Packed &out, const double *imu_sqrt, int mode = 0, int chain_lds = 0, bool plan_only = false, int coop_chunks = 0);
int pack_problem_data(const tcv_problem &p, Packed &out, const double *imu_sqrt, double *dst);
// Where the doubles of a window go: a Sink counts (no destination), writes into a buffer that was sized by a counting pass (the solve
// windows: all of a batch straight into one upload buffer), or appends to a vector (the marginalisation problems).
struct Sink {
    double *dst = nullptr;
    std::vector<double> *vec = nullptr;
    size_t n = 0;
    explicit Sink(double *d) : dst(d) {}
    explicit Sink(std::vector<double> &v) : vec(&v) {}
    void put(const double *s, size_t k) { if (vec) vec->insert(vec->end(), s, s + k); else if (dst) std::memcpy(dst + n, s, k * sizeof(double)); n += k; }
    void put1(double v) { if (vec) vec->push_back(v); else if (dst) dst[n] = v; n++; }
    void zeros(size_t k) { if (vec) vec->insert(vec->end(), k, 0.0); else if (dst) std::memset(dst + n, 0, k * sizeof(double)); n += k; }
};
// The record layouts that the solve and the marginalisation kernels both read (the marginalisation reads the solve batch's copy where it
// can: MargHdr::imu_abs, prior_abs), each with its one host writer (tcv_pack.cpp); prior_splice_kernel writes the first two on the device.
void put_imu_const(Sink &D, const tcv_imu_preintegration &q);      // IMU_CONST doubles: [dp 3 | dq 4 | dv 3 | ba 3 | bg 3 | sum_dt | dp_dba dp_dbg dq_dbg dv_dba dv_dbg 9 each | covariance 225]
void put_prior_region(Sink &D, const tcv_prior &pr, int k0);       // J0 rows k0 .. n - 1 (column-major) | r0[k0 ..] | x0; the prior is on the host (tcv_prior_host)
// one projection record [pts 6 | aux 8 (ProjectionTdFactor only)]; `first` is the window's first record, whose sqrt_info and loss all share
int put_proj_record(Sink &D, const ProjFac &f, const ProjFac &first);
// first failing window of a parallel packing pass, with the message of the thread that packed it (the message is thread-local)
struct PackErrors {
    std::vector<int> rcs, who;
    std::vector<std::string> msgs;
    PackErrors(int n, int nth) : rcs(n, TCV_OK), who(n, 0), msgs(nth) {}
    void note(int w, int t, int rc) { rcs[w] = rc; who[w] = t; if (rc != TCV_OK && msgs[t].empty()) msgs[t] = tcv_last_error(); }
    int first() const {      // TCV_OK, or that window's status with its message as the calling thread's error
        for (size_t w = 0; w < rcs.size(); w++)
            if (rcs[w] != TCV_OK) { if (!msgs[who[w]].empty()) set_error(msgs[who[w]]); return rcs[w]; }
        return TCV_OK;
    }
};
// plan-cache statistics (hits, misses, entries); tcv_pack.cpp
void plan_cache_stats(long long *hits, long long *misses, long long *entries);
void set_pack_reference(int on);
void pack_laps_print();      // TCV_DEBUG_PACK2=1: per-phase times of the packer since the last call, on stderr
bool pack_reference();
void cam_cache_stats(long long *hits, long long *misses);      // the camera halves of the plans (tcv_pack.cpp)
unsigned long long plan_content_hash(const PlanHdr &hdr, const PlanInts &ints);
}  // namespace tcv

#include "tcv_batch.h"      // struct tcv_batch: its parts and side states
