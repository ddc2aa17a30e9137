// Host side of the marginalisation (the kernel and its launchers: tcv_marg.hip; what the two share: tcv_marg.h): the packer that turns a
// marginalisation problem into the kernel's plan (pack_marg, in phases), the per-batch state behind tcv_batch::marg (MargState: attach, run, download)
// and the hand-out of the results as priors, host- or device-resident.
//
// Block order (the reference's is unordered_map / address dependent, marginalization_factor.cpp:176-194): dropped blocks in the order
// they were added to the problem, then kept blocks in that order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tcv_marg.h"

namespace tcv {

struct MargWindow {
    MargHdr hdr;
    std::vector<int> keep_block;      // marg-problem block index of every kept block (in mloc order)
    std::vector<int> keep_size, keep_idx, keep_goff;
    std::vector<double *> keep_addr;
    int m_total = 0;                  // all dropped tangent dims (landmarks included), the reference's m
    bool empty_keep = false;          // every block the factors touch is dropped (n = 0): nothing runs on the device, the result is the reference's
                                      // empty MarginalizationInfo (marginalization_factor.cpp:174-194 with n = pos - m = 0; carried into the next frame
                                      // by estimator.cpp:2040-2043, where its factor has no residuals and no blocks)
};
struct MargState : tcv::SideState {
    std::vector<MargWindow> win;
    void *d_input = nullptr;          // one allocation: [double pool | headers | int pool]
    MargHdr *d_hdr = nullptr;
    int *d_ipool = nullptr, *d_status = nullptr;      // d_status: per window [status | k0] (2 n ints): marginalisation status, leading zero rows of J0 | r0 (-1: NaN)
    double *d_dpool = nullptr, *d_out = nullptr, *d_scratch = nullptr;
    std::shared_ptr<DevBlob> out_blob;                // owns d_out: device-resident priors (tcv_batch_get_priors_device) keep it alive after the batch
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    size_t lds_bytes = 0;
    int grid = 0, nt = MARG_NT_WIDE;
    int *h_status_pre = nullptr;      // pinned: [status | k0] copied behind the kernel by tcv_marg_status_prefetch (valid once the batch's work is waited for)
    bool status_prefetched = false;
    bool ran = false;
    double *h_out = nullptr;          // pinned host copy of every window's result block (tcv_batch_download_priors), valid until the next run
    size_t h_stride = 0;              // doubles per window in h_out: MARG_OUT_STRIDE, or MARG_OUT_COMPACT (no A', b')
    std::vector<int> h_status;
    bool h_valid = false;
    ~MargState() override {
        (void)tcv::dev_free(d_input);      // (d_hdr, d_ipool, d_dpool point into d_input; d_status lives behind d_out in the result blob)
        out_blob.reset();                  // (d_out: freed when the last device-resident prior that reads it is gone)
        (void)tcv::dev_free(d_scratch);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        tcv::host_staging_release(h_out);
        tcv::host_staging_release(h_status_pre);
    }
};
static MargState *marg_of(const tcv_batch *b) { return static_cast<MargState *>(b->marg.get()); }

// The developer switches of the marginalisation, read once per attach / plan dump (the packer's and the launch shape's) or per run (the
// kernel's) and handed down -- per call, not once per process: the tests flip them between the batches of one process
struct MargSwitches {
    bool proj_serial = false, block_serial = false, own_imu = false, own_prior = false;      // the packer's (A/B checks of the kernel's shortcuts)
    bool nt_forced = false; int nt = 0, grid_cap = 0;                                        // the launch shape's (TCV_MARG_NT, TCV_MARG_GRID)
    bool debug = false;
    bool own_sqrt = false, eig_mm = false; int eig_flags = 0;                                // the run's
    static bool on(const char *k) { return getenv(k) != nullptr; }
    static int num(const char *k) { const char *v = getenv(k); return v ? atoi(v) : 0; }
    static MargSwitches for_attach() {
        MargSwitches s;
        s.proj_serial = on("TCV_MARG_PROJ_SERIAL"); s.block_serial = on("TCV_MARG_BLOCK_SERIAL"); s.own_imu = on("TCV_MARG_OWN_IMU"); s.own_prior = on("TCV_MARG_OWN_PRIOR");
        s.nt_forced = on("TCV_MARG_NT"); s.nt = num("TCV_MARG_NT"); s.grid_cap = num("TCV_MARG_GRID"); s.debug = on("TCV_DEBUG");
        return s;
    }
    static MargSwitches for_run() {
        MargSwitches s;
        s.own_sqrt = on("TCV_MARG_OWN_SQRT"); s.eig_mm = on("TCV_MARG_EIG_MM"); s.eig_flags = num("TCV_MARG_EIG_FLAGS");
        return s;
    }
};

// The LDS carve of one window, in doubles: [P: packed A, later A' and its eigenvectors | R2: staging records (64 x 43: a ProjectionTdFactor
// record is 2 x 21 + 1), later Amm + V, later the packed reflectors | b | x | rot | lam | landmark row | eigen vectors].  This is the HOST
// copy of the carve at the top of marg_kernel (tcv_marg.hip, "LDS carve"): the two must be changed together -- the kernel keeps its own
// arithmetic because sharing a function with it moves its register allocation.  cb_off < 0: the window has no C buffer (yet).
struct MargLds {
    int p;                      // doubles of region P = offset of R2
    int r2;                     // doubles of region R2
    int cb_in_r2;               // doubles C adds to R2 (cb_off behind the staging records), 0 when it lies in P or there is none
    int cb_off_p, cb_off_r2;    // where C may go: in the part of P the packed A does not use (-1: no room), or behind the staging records
    size_t total;
    bool fits;                  // one window of these sizes runs in one piece: m, n within the eigen-solvers' limits and the carve within a CU's LDS
};
static MargLds marg_lds_layout(int pos, int m, int n, int nx, int cb_off, int cb_stride) {
    MargLds L;
    const int me = m + (m & 1), ne = n + (n & 1), npk = pos * (pos + 1) / 2, apk = (npk + 1) & ~1;
    const int r1 = std::max(npk, ne * (ne + 1)), need = MARG_CB_LM * cb_stride + 2 * MARG_CB_LM;
    L.p = (r1 + 1) & ~1;
    L.cb_off_p = r1 - apk >= need ? apk : -1;
    L.cb_off_r2 = L.p + (int)MARG_STAGE;
    L.cb_in_r2 = (cb_off >= 0 && cb_off >= L.p) ? need : 0;
    L.r2 = std::max(std::max((int)MARG_STAGE + L.cb_in_r2, me * (me + 1) + std::max(me * (me + 1), m * (n + 1))), (n - 2) * (n - 1) / 2 + 1);
    L.total = (size_t)L.p + ((L.r2 + 1) & ~1) + MARG_MAX_POS + ((nx + 7) & ~7) + 160 + MARG_MAX_N + MARG_MAX_POS + 8 + MARG_SM;
    L.fits = m <= MARG_MAX_M && n <= MARG_MAX_N && L.total <= (size_t)LDS_DOUBLES;
    return L;
}

// ---- the packer: one marginalisation problem -> header, int records, double records ------------------------------------------------
// The blocks the factors touch, in the order they were added to the problem (c = 0 .. nblk - 1), and their [m | n] tangent numbering.
// MarginalizationInfo knows nothing about SetParameterBlockConstant: a constant block (para_Ex_Pose with ESTIMATE_EXTRINSIC = 0,
// estimator.cpp:1694-1698) is kept / dropped like any other and its Jacobian columns are accumulated (marginalization_factor.cpp:89-108,
// :176-194), so the prior of the shipped EuRoC configuration has n = 75 too.
struct MargBlocks {
    std::vector<int> id_of;                    // problem block -> c, -1: untouched
    std::vector<int> orig, goff, mloc;         // per c: problem block, offset in x, tangent column (-2 - l: eliminated landmark l, block mode)
    std::vector<char> dropped;                 // per problem block
    // marginalised inverse depths: size-1 blocks that only ever appear as 4th block of projection factors.  When the dropped set is too
    // large for the LDS-resident eigen-solver (a 150-feature front end anchors far more than 49 landmarks in the oldest frame) they are
    // eliminated by scalar pivots (block mode) and only the frame part goes through the eigen step.
    std::vector<char> pivot_lm;                // per problem block: such a block, dropped
    std::vector<int> lm_id;                    // per problem block: its index among the eliminated landmarks (block mode), -1
    int nblk = 0, nx = 0, m_all = 0, n_all = 0, n_lm_drop = 0;      // m_all, n_all: dropped / kept tangent dims, landmarks included
    bool block_mode = false;
    int m = 0, n = 0, pos = 0;                 // the numbering: m dims through the eigen step, n kept
};
static int tangent_size(const ParamBlock &pb) { return pb.kind == KIND_POSE ? 6 : pb.size; }

static int marg_classify(const tcv_problem &p, double *const *drop, int ndrop, MargBlocks &B) {
    const int nb = (int)p.blocks.size();
    if (!p.line.empty()) { set_error("line factors are not marginalised (estimator.cpp:1992 `if (0)`)"); return TCV_ERR_UNSUPPORTED; }
    if (p.prior.size() > 1) { set_error("more than one marginalisation factor"); return TCV_ERR_UNSUPPORTED; }
    // touched: by any factor; other_use: by anything but the 4th slot of a projection factor
    std::vector<char> touched(nb, 0), is_lm(nb, 0), other_use(nb, 0);
    for (auto &f : p.imu) for (int k = 0; k < 4; k++) touched[f.b[k]] = other_use[f.b[k]] = 1;
    for (auto &f : p.proj) {
        for (int k = 0; k < 3; k++) touched[f.b[k]] = other_use[f.b[k]] = 1;
        touched[f.b[3]] = is_lm[f.b[3]] = 1;
        if (f.btd >= 0) touched[f.btd] = other_use[f.btd] = 1;
    }
    for (auto &f : p.prior) for (int b : f.b) touched[b] = other_use[b] = 1;
    B.dropped.assign(nb, 0);
    for (int k = 0; k < ndrop; k++) {
        const int bd = p.index.find(drop[k]);
        if (bd < 0) { set_error("marginalize: dropped block is not part of the problem"); return TCV_ERR_INVALID; }
        if (touched[bd]) B.dropped[bd] = 1;
    }
    B.id_of.assign(nb, -1); B.pivot_lm.assign(nb, 0);
    for (int b = 0; b < nb; b++) {
        if (!touched[b]) continue;
        const ParamBlock &pb = p.blocks[b];
        B.id_of[b] = (int)B.orig.size();
        B.orig.push_back(b); B.goff.push_back(B.nx);
        B.nx += pb.size;
        if (!B.dropped[b]) { B.n_all += tangent_size(pb); continue; }
        B.m_all += tangent_size(pb);
        if (is_lm[b] && !other_use[b] && pb.size == 1) { B.pivot_lm[b] = 1; B.n_lm_drop++; }
    }
    B.nblk = (int)B.orig.size();
    return TCV_OK;
}
// tangent columns: dropped blocks in problem order (block mode: the pivot landmarks get no column), then the kept ones, which are also
// the blocks of the prior this marginalisation makes (mw.keep_*)
static void marg_number(const tcv_problem &p, MargBlocks &B, MargWindow &mw) {
    const int nb = (int)p.blocks.size();
    B.mloc.assign(B.nblk, -1); B.lm_id.assign(nb, -1);
    int pos = 0, n_lm = 0;
    for (int c = 0; c < B.nblk; c++) {
        const int b = B.orig[c];
        if (!B.dropped[b]) continue;
        if (B.block_mode && B.pivot_lm[b]) { B.lm_id[b] = n_lm; B.mloc[c] = -2 - n_lm; n_lm++; continue; }
        B.mloc[c] = pos; pos += tangent_size(p.blocks[b]);
    }
    B.m = pos;
    mw.keep_block.clear(); mw.keep_size.clear(); mw.keep_idx.clear(); mw.keep_addr.clear(); mw.keep_goff.clear();
    for (int c = 0; c < B.nblk; c++) {
        const ParamBlock &pb = p.blocks[B.orig[c]];
        if (B.dropped[B.orig[c]]) continue;
        B.mloc[c] = pos;
        mw.keep_block.push_back(c); mw.keep_size.push_back(pb.size); mw.keep_idx.push_back(pos); mw.keep_addr.push_back(pb.addr);
        mw.keep_goff.push_back(B.goff[c]);
        pos += tangent_size(pb);
    }
    B.pos = pos; B.n = pos - B.m;
}
// where the current value of each block lives in the solve's state vector (-1: nowhere)
static std::vector<int> marg_state_sources(const tcv_problem &p, const MargBlocks &B, const tcv_problem *solve_p, const Packed *solve_pk) {
    std::vector<int> xsrc(B.nblk, -1);
    if (!solve_p || !solve_pk) return xsrc;
    std::unordered_map<double *, int> off;
    int o = 0;
    for (int blkid : solve_pk->cam_block) { off[solve_p->blocks[blkid].addr] = o; o += solve_p->blocks[blkid].size; }
    for (int blkid : solve_pk->lm_block) { off[solve_p->blocks[blkid].addr] = o; o += 1; }
    for (int c = 0; c < B.nblk; c++) { auto it = off.find(p.blocks[B.orig[c]].addr); if (it != off.end()) xsrc[c] = it->second; }
    return xsrc;
}
// the (single) IMU factor's index among the solve problem's IMU factors: the same pre-integration (MARGIN_OLD: the factor between frames
// 0 and 1), whose sqrt_info the solve computed and whose constants lie in the solve batch's pool; -1: none
static int marg_sqrt_source(const tcv_problem &p, const tcv_problem *solve_p) {
    if (p.imu.size() != 1 || !solve_p) return -1;
    for (size_t g = 0; g < solve_p->imu.size(); g++) {
        const bool same = p.imu[0].dev ? solve_p->imu[g].dev == p.imu[0].dev
                                       : (!solve_p->imu[g].dev && std::memcmp(&solve_p->imu[g].pre, &p.imu[0].pre, sizeof(tcv_imu_preintegration)) == 0);
        if (same) return (int)g;
    }
    return -1;
}

// The order the point factors are evaluated in and, for the chunked block path (MargHdr::n_pchunk), how they are cut and grouped.
struct MargFactorPlan {
    std::vector<int> porder;      // position -> projection factor (block mode: sorted by landmark)
    int td_blk = -1, proj_disjoint = 1;
    bool chunked = false;         // chunks of whole landmarks, the landmarks' couplings eliminated by one rank-16 update per chunk
    std::vector<int> chunks;      // per chunk: first factor, factors, eliminated landmarks, offset of its group table in pgrp
    std::vector<int> plm;         // per factor: index of its landmark among the chunk's eliminated landmarks, -1: a regular column
    std::vector<int> pgrp;        // the chunks' group tables (MargHdr::o_pgrp)
};
// cuts the sorted factors into chunks of whole landmarks (<= 64 factors, <= MARG_CB_LM eliminated landmarks); false: a landmark with more
// than 64 factors is eliminated -- the factor-by-factor path takes the window
static bool marg_cut_chunks(const tcv_problem &p, const MargBlocks &B, MargFactorPlan &F) {
    const std::vector<int> &porder = F.porder;
    std::vector<int> &chunks = F.chunks;
    F.plm.assign(porder.size(), -1);
    size_t i = 0;
    while (i < porder.size()) {
        const size_t c0 = i;
        int nl = 0;
        while (i < porder.size()) {
            size_t j = i;      // the factors of one landmark: [i, j)
            const int lmb = p.proj[porder[i]].b[3];
            while (j < porder.size() && p.proj[porder[j]].b[3] == lmb) j++;
            const bool elim = B.lm_id[lmb] >= 0;
            if (i > c0 && (j - c0 > 64 || (elim && nl == MARG_CB_LM))) break;
            if (j - c0 > 64) { j = c0 + 64; if (elim) { chunks.clear(); i = porder.size(); break; } }      // (a landmark with more than 64 factors: old path)
            for (size_t q = i; q < j; q++) F.plm[q] = elim ? nl : -1;
            if (elim) nl++;
            i = j;
        }
        if (i == porder.size() && chunks.empty() && c0 != 0) break;
        chunks.push_back((int)c0); chunks.push_back((int)(i - c0)); chunks.push_back(nl); chunks.push_back(0);
    }
    return !chunks.empty() || porder.empty();
}
// one chunk's group table, appended to pgrp: [frames nfr | landmark runs nlg | 1 if every factor shares its first pose and its extrinsic
// block | length | (first, count) x nfr into the list at the end | (first factor, count) x nlg | the chunk's factors grouped by their
// second pose, factor order inside a group]
static void marg_group_chunk(const tcv_problem &p, const std::vector<int> &porder, int c0, int cn, std::vector<int> &pgrp) {
    std::vector<int> keys, runs;
    std::vector<std::vector<int>> members;
    bool uniform = true;
    for (int q = 0; q < cn; q++) {
        const ProjFac &f = p.proj[porder[c0 + q]];
        size_t k = 0;
        while (k < keys.size() && keys[k] != f.b[1]) k++;
        if (k == keys.size()) { keys.push_back(f.b[1]); members.emplace_back(); }
        members[k].push_back(q);
        if (q == 0 || p.proj[porder[c0 + q - 1]].b[3] != f.b[3]) { runs.push_back(q); runs.push_back(0); }
        runs.back()++;
        if (f.b[0] != p.proj[porder[c0]].b[0] || f.b[2] != p.proj[porder[c0]].b[2]) uniform = false;
    }
    const size_t h0 = pgrp.size();
    pgrp.push_back((int)keys.size()); pgrp.push_back((int)runs.size() / 2); pgrp.push_back(uniform ? 1 : 0); pgrp.push_back(0);
    int off = 0;
    for (auto &mbr : members) { pgrp.push_back(off); pgrp.push_back((int)mbr.size()); off += (int)mbr.size(); }
    pgrp.insert(pgrp.end(), runs.begin(), runs.end());
    for (auto &mbr : members) pgrp.insert(pgrp.end(), mbr.begin(), mbr.end());
    pgrp[h0 + 3] = (int)(pgrp.size() - h0);
}
static int marg_plan_factors(const tcv_problem &p, const MargBlocks &B, const MargSwitches &sw, MargFactorPlan &F) {
    const int nb = (int)p.blocks.size();
    F.porder.resize(p.proj.size());
    for (size_t i = 0; i < F.porder.size(); i++) F.porder[i] = (int)i;
    if (B.block_mode) {
        for (auto &f : p.proj)
            if (B.dropped[f.b[3]] && B.lm_id[f.b[3]] < 0) { set_error("marginalize: dropped inverse depth shared with a non-projection factor"); return TCV_ERR_UNSUPPORTED; }
        std::stable_sort(F.porder.begin(), F.porder.end(), [&](int a, int b2) { return p.proj[a].b[3] < p.proj[b2].b[3]; });
    }
    for (size_t k = 0; k < p.proj.size(); k++) {
        if (p.proj[k].btd != p.proj[0].btd) { set_error("projection factors must all be ProjectionTdFactors on one Td block, or none"); return TCV_ERR_UNSUPPORTED; }
        if (p.proj[k].btd >= 0) F.td_blk = B.id_of[p.proj[k].btd];
    }
    std::vector<char> as_i(nb, 0), as_j(nb, 0);
    for (auto &f : p.proj) { as_i[f.b[0]] = 1; as_j[f.b[1]] = 1; }
    for (int c = 0; c < nb; c++) if (as_i[c] && as_j[c]) F.proj_disjoint = 0;
    if (sw.proj_serial) F.proj_disjoint = 0;      // A/B checks: the factor-by-factor accumulation
    if (!(B.block_mode && F.proj_disjoint && F.td_blk < 0 && !sw.block_serial)) return TCV_OK;
    if (!(F.chunked = marg_cut_chunks(p, B, F))) return TCV_OK;
    if (sw.debug) {
        fprintf(stderr, "[tcv] marg plan: %d projection factors in %d chunks (factors, eliminated landmarks):", (int)F.porder.size(), (int)F.chunks.size() / 4);
        for (size_t c = 0; c + 3 < F.chunks.size(); c += 4) fprintf(stderr, " (%d, %d)", F.chunks[c + 1], F.chunks[c + 2]);
        fprintf(stderr, "\n");
    }
    for (size_t c = 0; c + 3 < F.chunks.size(); c += 4) {
        F.chunks[c + 3] = (int)F.pgrp.size();
        marg_group_chunk(p, F.porder, F.chunks[c], F.chunks[c + 1], F.pgrp);
    }
    return TCV_OK;
}

// the int records of the window behind I (offsets in H relative to the window's first int), and where C goes in the LDS
static int marg_write_ints(const tcv_problem &p, const MargBlocks &B, const std::vector<int> &xsrc, const MargFactorPlan &F, MargHdr &H, std::vector<int> &I) {
    const size_t i0 = I.size();
    auto imark = [&]() { return (int)(I.size() - i0); };
    H.o_blk = imark();
    for (int c = 0; c < B.nblk; c++) { const ParamBlock &pb = p.blocks[B.orig[c]]; I.push_back(pb.size); I.push_back(B.goff[c]); I.push_back(B.mloc[c]); I.push_back(pb.kind); I.push_back(xsrc[c]); }
    H.o_imu = imark();
    for (auto &f : p.imu) for (int k = 0; k < 4; k++) I.push_back(B.id_of[f.b[k]]);
    H.o_proj = imark();
    for (int k2 : F.porder) for (int k = 0; k < 4; k++) I.push_back(B.id_of[p.proj[k2].b[k]]);
    H.o_plast = imark();      // block mode: 1 = last factor of its (eliminated) landmark
    for (size_t i = 0; i < F.porder.size(); i++) {
        const int lmb = p.proj[F.porder[i]].b[3];
        I.push_back(B.block_mode && B.lm_id[lmb] >= 0 && (i + 1 == F.porder.size() || p.proj[F.porder[i + 1]].b[3] != lmb) ? 1 : 0);
    }
    H.cb_off = -1; H.cb_stride = 0; H.n_pchunk = 0; H.o_pchunk = imark(); H.o_plm = imark();
    if (F.chunked) {
        H.n_pchunk = (int)F.chunks.size() / 4;
        H.o_pchunk = imark(); I.insert(I.end(), F.chunks.begin(), F.chunks.end());
        H.o_plm = imark(); I.insert(I.end(), F.plm.begin(), F.plm.end());
        H.o_pgrp = imark(); I.insert(I.end(), F.pgrp.begin(), F.pgrp.end());
        H.cb_stride = (B.pos + 15) & ~15;
        const MargLds L = marg_lds_layout(B.pos, B.m, B.n, B.nx, -1, H.cb_stride);
        H.cb_off = L.cb_off_p >= 0 ? L.cb_off_p : L.cb_off_r2;
    }
    H.o_prior = imark();
    std::vector<int> pcol;
    if (const tcv_prior *pr = p.prior.empty() ? nullptr : p.prior[0].prior) {
        if (pr->n > 128) { set_error("prior with more than 128 rows"); return TCV_ERR_TOO_LARGE; }
        H.prior_n = pr->n; H.prior_nblk = (int)pr->size.size(); H.prior_xsize = pr->xsize;
        pcol.assign(pr->n, -1);
        for (int k = 0; k < H.prior_nblk; k++) {
            const int c = B.id_of[p.prior[0].b[k]];
            I.push_back(c); I.push_back(pr->idx[k]); I.push_back(pr->size[k]); I.push_back(pr->xoff[k]);
            const int local = pr->size[k] == 7 ? 6 : pr->size[k];
            for (int j = 0; j < local; j++) if (pr->idx[k] + j < pr->n) pcol[pr->idx[k] + j] = B.mloc[c] < 0 ? -1 : B.mloc[c] + j;
        }
    }
    H.o_pcol = imark();
    I.insert(I.end(), pcol.begin(), pcol.end());
    return TCV_OK;
}

// the double records behind D: x, then the factors' constants -- or, where the solve batch's data pool holds the same record (the IMU
// factor's, the prior's), its place there (MargHdr::imu_abs, prior_abs) and nothing here
static int marg_write_doubles(const tcv_problem &p, const MargBlocks &B, const MargFactorPlan &F, const MargSwitches &sw,
                              const tcv_problem *solve_p, const Packed *solve_pk, MargHdr &H, std::vector<double> &D) {
    const size_t d0 = D.size();
    auto dmark = [&]() { return (int)(D.size() - d0); };
    H.d_x = dmark();
    for (int c = 0; c < B.nblk; c++) { const ParamBlock &pb = p.blocks[B.orig[c]]; D.insert(D.end(), pb.addr, pb.addr + pb.size); }
    H.d_imu = dmark();
    Sink DS(D);      // the records shared with the solve windows: one writer each (tcv_host.h)
    H.imu_abs = -1;
    if (H.sqrt_src >= 0 && solve_pk && !sw.own_imu) H.imu_abs = solve_pk->win.dbase + solve_pk->win.d_imu + (long long)H.sqrt_src * IMU_CONST;
    for (auto &f : p.imu) {
        if (H.imu_abs >= 0) break;
        if (f.dev) { if (int rc = tcv_preint_host(f.dev)) return rc; }      // (no shared copy to read from: the numbers are needed here)
        put_imu_const(DS, f.dev ? f.dev->pod : f.pre);
    }
    H.d_proj = dmark();
    for (int k : F.porder) {
        const ProjFac &f = p.proj[k];
        if (int rc = put_proj_record(DS, f, p.proj[F.porder[0]])) return rc;
        if (p.blocks[f.b[3]].size != 1) { set_error("projection factor: 4th block must be an inverse depth"); return TCV_ERR_UNSUPPORTED; }
    }
    const double psi = p.proj.empty() ? 0.0 : p.proj[F.porder[0]].sqrt_info, pla = p.proj.empty() ? 0.0 : p.proj[F.porder[0]].loss_a;
    H.d_prior = dmark();
    H.prior_abs = -1;
    const tcv_prior *pr = p.prior.empty() ? nullptr : p.prior[0].prior;
    if (pr && solve_p && solve_pk && !solve_p->prior.empty() && solve_p->prior[0].prior == pr && solve_pk->hdr.prior_n == pr->n && !sw.own_prior)
        { H.prior_abs = solve_pk->win.dbase + solve_pk->win.d_prior; H.prior_k0 = solve_pk->prior_k0_deferred ? -1 : solve_pk->win.prior_k0; }      // the same record: put_prior_region, or the splice kernel's copy of it
    else if (pr) {
        if (int rc = tcv_prior_host(pr)) return rc;      // (a device-resident prior that the solve problem does not share: its numbers are needed here)
        H.prior_k0 = prior_keep_zero_rows() ? 0 : prior_zero_rows(pr->J0.data(), pr->r0.data(), pr->n);
        put_prior_region(DS, *pr, H.prior_k0);
    }
    H.d_misc = dmark();
    D.insert(D.end(), p.G, p.G + 3); D.push_back(psi); D.push_back(pla); D.push_back(0.0); D.push_back(p.td_TR); D.push_back(p.td_ROW);
    if (D.size() & 1) D.push_back(0.0);
    return TCV_OK;
}

enum { MARG_PACK_EMPTY_KEEP = 1 };      // pack_marg: the marginalisation keeps nothing (MargWindow::empty_keep); not an error
static int pack_marg(const tcv_problem &p, double *const *drop, int ndrop, const tcv_problem *solve_p, const Packed *solve_pk, const MargSwitches &sw,
                     MargWindow &mw, std::vector<int> &I, std::vector<double> &D) {
    MargBlocks B;
    if (int rc = marg_classify(p, drop, ndrop, B)) return rc;
    // one-piece eigen-decomposition of A_mm (the reference's) whenever it fits the LDS, block mode otherwise
    B.block_mode = !marg_lds_layout(B.m_all + B.n_all, B.m_all, B.n_all, B.nx, -1, 0).fits && B.n_lm_drop > 0;
    marg_number(p, B, mw);
    mw.m_total = B.m_all;
    // nothing kept -- every touched block is dropped, or the problem holds no factor at all (frame 0 without a prior, its IMU factor left out,
    // nothing anchored in it): the reference's marginalize() runs with n = 0 (and m = 0 in the second case) and leaves an empty MarginalizationInfo
    if (B.n < 1) { mw.empty_keep = true; return MARG_PACK_EMPTY_KEEP; }      // (the caller writes a header the kernel skips)
    if (B.m_all < 1) { set_error("marginalize: none of the dropped blocks is touched by a factor (m = 0, n > 0: the kernel has no path without a dropped block)"); return TCV_ERR_INVALID; }
    if (B.block_mode && B.m < 1) { set_error("marginalize: block mode needs a non-landmark block in the dropped set"); return TCV_ERR_UNSUPPORTED; }
    if (B.m > MARG_MAX_M || B.n > MARG_MAX_N || B.nx > MARG_MAX_X || p.imu.size() > 16) {
        set_error("marginalisation too large for the LDS-resident kernel (m <= 64, n <= 80)");
        return TCV_ERR_TOO_LARGE;
    }
    MargFactorPlan F;
    if (int rc = marg_plan_factors(p, B, sw, F)) return rc;
    MargHdr &H = mw.hdr;
    std::memset(&H, 0, sizeof H);
    H.nblk = B.nblk; H.pos = B.pos; H.m = B.m; H.n = B.n; H.nx = B.nx;
    H.n_imu = (int)p.imu.size(); H.n_proj = (int)p.proj.size();
    H.ibase = (long long)I.size(); H.dbase = (long long)D.size();
    H.block_mode = B.block_mode ? 1 : 0; H.td_blk = F.td_blk; H.proj_disjoint = F.proj_disjoint;
    H.sqrt_src = marg_sqrt_source(p, solve_p);
    if (int rc = marg_write_ints(p, B, marg_state_sources(p, B, solve_p, solve_pk), F, H, I)) return rc;
    return marg_write_doubles(p, B, F, sw, solve_p, solve_pk, H, D);
}

int DevBlob::wait_ready(hipStream_t consumer) const {
    if (!ready) return TCV_OK;
    const hipError_t e = hipStreamWaitEvent(consumer, ready, 0);
    return e == hipSuccess ? TCV_OK : hip_fail(e, "hipStreamWaitEvent (device-resident input)");
}
int DevBlob::sync_ready() const {
    if (!ready) return TCV_OK;
    const hipError_t e = hipEventSynchronize(ready);
    return e == hipSuccess ? TCV_OK : hip_fail(e, "hipEventSynchronize (device-resident input)");
}
DevBlob::~DevBlob() {
    if (ready) { (void)hipEventSynchronize(ready); (void)hipEventDestroy(ready); }      // (the buffer goes back to a pool: its producer must be done)
    if (!p) return;
    int cur = 0;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != dev;
    if (sw) (void)hipSetDevice(dev);      // (the free list is per device)
    (void)dev_free(p);
    if (sw) (void)hipSetDevice(cur);
}

}  // namespace tcv
using namespace tcv;

// materialises a device-resident prior on the host (export / checkpoint, or a consumer that needs the numbers: a marginalisation problem
// that does not share its prior with the solve problem)
int tcv_prior_host(const tcv_prior *pr) {
    if (!pr) return TCV_ERR_INVALID;
    std::lock_guard<std::mutex> g(pr->mu);
    if (pr->host) return TCV_OK;
    const int n = pr->n;
    std::vector<double> o(MARG_OUT_COMPACT);
    int cur = 0;
    const bool sw = hipGetDevice(&cur) == hipSuccess && pr->dev && cur != pr->dev->dev;
    if (sw) (void)hipSetDevice(pr->dev->dev);
    if (pr->dev) if (const int rcw = pr->dev->sync_ready()) { if (sw) (void)hipSetDevice(cur); return rcw; }
    const int rcd = tcv::staged_download(o.data(), pr->d_block, sizeof(double) * MARG_OUT_COMPACT, "download of a device-resident prior");
    if (sw) (void)hipSetDevice(cur);
    if (rcd != TCV_OK) return rcd;
    pr->J0.assign(o.begin() + MARG_OUT_J0, o.begin() + MARG_OUT_J0 + (size_t)n * n);
    pr->r0.assign(o.begin() + MARG_OUT_R0, o.begin() + MARG_OUT_R0 + n);
    pr->x0.clear();
    for (size_t k = 0; k < pr->size.size(); k++) for (int i = 0; i < pr->size[k]; i++) pr->x0.push_back(o[MARG_OUT_X + pr->x_goff[k] + i]);
    pr->host = true;
    return TCV_OK;
}

int tcv_marg_plan(const tcv_problem &p, double *const *drop, int ndrop, const tcv_problem *solve_p, const Packed *solve_pk,
                  std::vector<int> &ints, std::vector<double> &doubles) {
    MargWindow mw;
    std::vector<int> I;
    ints.clear(); doubles.clear();
    const int rc = pack_marg(p, drop, ndrop, solve_p, solve_pk, MargSwitches::for_attach(), mw, I, doubles);
    if (rc == MARG_PACK_EMPTY_KEEP) { doubles.clear(); return TCV_OK; }
    if (rc != TCV_OK) return rc;
    ints.resize(sizeof(MargHdr) / sizeof(int));
    std::memcpy(ints.data(), &mw.hdr, sizeof(MargHdr));
    ints.insert(ints.end(), I.begin(), I.end());
    return TCV_OK;
}
extern "C" int tcv_marg_lds_layout(int pos, int m, int n, int nx, int cb_off, int cb_stride, int *out7) {
    if (!out7 || pos < 0 || m < 0 || n < 0 || nx < 0 || cb_stride < 0) return TCV_ERR_INVALID;
    const MargLds L = marg_lds_layout(pos, m, n, nx, cb_off, cb_stride);
    const int v[7] = {L.p, L.r2, L.cb_in_r2, L.cb_off_p, L.cb_off_r2, (int)L.total, L.fits ? 1 : 0};
    std::memcpy(out7, v, sizeof v);
    return TCV_OK;
}

// ---- tcv_marg_attach: pack on the host threads, lay the pools end to end, decide the launch shape, upload ---------------------------
// The windows are packed by host threads, each into its own int / double pools (contiguous window ranges); the pools are then laid end
// to end in one pinned upload buffer and the headers' pool offsets shifted accordingly.
struct MargPools {
    int n, nth;
    std::vector<std::vector<int>> I;
    std::vector<std::vector<double>> D;
    std::vector<size_t> ib, db;      // first int / double of thread t's pools in the batch's pools (nth + 1 entries)
    MargPools(int n_, int nth_) : n(n_), nth(nth_), I(nth_), D(nth_), ib(nth_ + 1, 0), db(nth_ + 1, 0) {}
    int first(int t) const { return (int)((long long)n * t / nth); }      // thread t packs windows [first(t), first(t + 1))
};
// an empty header (nblk = 0), which the kernel skips: a window of the batch that is not marginalised, or whose marginalisation keeps nothing
static void marg_skip_header(MargHdr &H, size_t ibase, size_t dbase, int w) {
    std::memset(&H, 0, sizeof H);
    H.ibase = (long long)ibase; H.dbase = (long long)dbase;
    H.sqrt_src = -1; H.prior_abs = -1; H.imu_abs = -1; H.cb_off = -1; H.td_blk = -1; H.solve_window = w;
}
static int marg_pack_windows(tcv_batch *b, tcv_problem *const *marg_problems, double *const *const *marg_drop, const int *marg_num_drop,
                             const MargSwitches &sw, MargState *s, MargPools &P) {
    std::vector<int> rcs(P.nth, TCV_OK);
    std::vector<std::string> msgs(P.nth);
    tcv::parallel_run(P.nth, [&](int t) {
        std::vector<int> &I = P.I[t];
        std::vector<double> &D = P.D[t];
        for (int w = P.first(t); w < P.first(t + 1); w++) {
            const size_t i0 = I.size(), d0 = D.size();
            const int rc = marg_problems[w] ? pack_marg(*marg_problems[w], marg_drop[w], marg_num_drop[w], b->in.problems[w], &b->in.packed[w], sw, s->win[w], I, D)
                                            : (int)MARG_PACK_EMPTY_KEEP;      // (not marginalised: skipped alike, but MargWindow::empty_keep stays false)
            if (rc == MARG_PACK_EMPTY_KEEP) { I.resize(i0); D.resize(d0); marg_skip_header(s->win[w].hdr, i0, d0, w); continue; }
            if (rc != TCV_OK) { rcs[t] = rc; msgs[t] = tcv_last_error(); return; }
            s->win[w].hdr.solve_window = w;
        }
    });
    for (int t = 0; t < P.nth; t++) if (rcs[t] != TCV_OK) { if (!msgs[t].empty()) set_error(msgs[t]); return rcs[t]; }
    return TCV_OK;
}
// shifts every header's pool offsets to the batch's pools and finds the LDS bytes the largest window needs
static int marg_concat(MargState *s, MargPools &P, std::vector<MargHdr> &hdrs, size_t &lds_bytes) {
    for (int t = 0; t < P.nth; t++) { P.ib[t + 1] = P.ib[t] + P.I[t].size(); P.db[t + 1] = P.db[t] + P.D[t].size(); }
    lds_bytes = 0;
    for (int t = 0; t < P.nth; t++)
        for (int w = P.first(t); w < P.first(t + 1); w++) {
            MargHdr &H = s->win[w].hdr;
            H.ibase += (long long)P.ib[t]; H.dbase += (long long)P.db[t];
            hdrs[w] = H;
            if (H.nblk == 0) continue;
            const size_t need = marg_lds_layout(H.pos, H.m, H.n, H.nx, H.cb_off, H.cb_stride).total * 8;
            if (need > (size_t)LDS_DOUBLES * 8) { set_error("marginalisation does not fit LDS"); return TCV_ERR_TOO_LARGE; }
            lds_bytes = std::max(lds_bytes, need);
        }
    return TCV_OK;
}
// one pinned staging buffer, one device blob: [double pool | headers | int pool]
struct MargBlobLayout {
    size_t o_hdr, o_int, bytes;
    MargBlobLayout(size_t d_total, size_t i_total, size_t nhdr) {
        auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        o_hdr = up16(sizeof(double) * std::max<size_t>(1, d_total)); o_int = up16(o_hdr + sizeof(MargHdr) * nhdr);
        bytes = up16(o_int + sizeof(int) * std::max<size_t>(1, i_total));
    }
};
static void marg_fill_staging(char *h_in, const MargBlobLayout &lay, const MargPools &P, const std::vector<MargHdr> &hdrs) {
    int *h_I = (int *)(h_in + lay.o_int);
    double *h_D = (double *)h_in;
    std::memcpy(h_in + lay.o_hdr, hdrs.data(), sizeof(MargHdr) * hdrs.size());
    tcv::parallel_run(P.nth, [&](int t) {
        if (!P.I[t].empty()) std::memcpy(h_I + P.ib[t], P.I[t].data(), sizeof(int) * P.I[t].size());
        if (!P.D[t].empty()) std::memcpy(h_D + P.db[t], P.D[t].data(), sizeof(double) * P.D[t].size());
    });
}
// more windows than CUs and every window within half a CU's LDS: two 256-thread workgroups per CU; otherwise one of 512 threads
static int marg_launch_shape(const tcv_batch *b, const MargSwitches &sw, size_t lds_bytes, MargState *s) {
    const int n_cu = b->shape.n_cu;      // (of the batch's device: tcv_batch_create sets it before anything attaches)
    const size_t half = (size_t)LDS_DOUBLES * 4;
    const bool pair = sw.nt_forced ? sw.nt == MARG_NT_PAIR : (b->in.n > n_cu && lds_bytes <= half);
    if (pair && lds_bytes > half) { set_error("TCV_MARG_NT=256: the batch does not fit 80 KB of LDS per window"); return TCV_ERR_TOO_LARGE; }
    s->nt = pair ? MARG_NT_PAIR : MARG_NT_WIDE;
    s->lds_bytes = pair ? half : lds_bytes;
    s->grid = std::min(b->in.n, pair ? 2 * n_cu : n_cu);
    if (sw.grid_cap > 0) s->grid = std::min(s->grid, sw.grid_cap);      // tuning experiments (one workgroup per CU: TCV_MARG_GRID=256)
    return TCV_OK;
}
// device buffers and the one asynchronous copy of the staged input on the calling thread's stream
static int marg_upload(tcv_batch *b, MargState *s, tcv::StagedTransfer &staged, const MargBlobLayout &lay) {
    hipStream_t ust = staged.st;
    const size_t out_doubles = std::max<size_t>(1, (size_t)b->in.n * MARG_OUT_STRIDE);
    hipError_t e_ = tcv::dev_malloc(&s->d_input, lay.bytes);
    if (e_ == hipSuccess) { staged.issued(); e_ = hipMemcpyAsync(s->d_input, staged.host, lay.bytes, hipMemcpyHostToDevice, ust); }
    // result blocks and, behind them, [status | k0] of every window: one buffer, kept alive by the device-resident priors that read it
    if (e_ == hipSuccess) e_ = tcv::dev_malloc((void **)&s->d_out, sizeof(double) * out_doubles + sizeof(int) * 2 * (size_t)b->in.n);
    if (e_ == hipSuccess) { s->out_blob = std::make_shared<DevBlob>(); s->out_blob->p = s->d_out; (void)hipGetDevice(&s->out_blob->dev); s->d_status = (int *)(s->d_out + out_doubles); }
    if (e_ == hipSuccess) e_ = tcv::dev_malloc((void **)&s->d_scratch, sizeof(double) * (size_t)s->grid * MARG_SCR_STRIDE);
    if (e_ == hipSuccess) e_ = hipMemsetAsync(s->d_status, 0xff, sizeof(int) * 2 * b->in.n, ust);
    // No wait for the upload: the native estimator attaches the problems while the batch's SOLVE runs on this very stream, and a wait here
    // is a wait for that kernel (a caller that overlaps another group's host work with it -- tcv_estimators_optimize_begin -- lost the whole
    // overlap to it).  The batch notes the stream (a later launch on another stream is ordered behind the upload by an event,
    // BatchFlight::enter); the pinned staging buffer is parked until this thread's next wait on the stream.
    if (e_ == hipSuccess && ust != nullptr) {
        if (int rce = b->flight.enter(ust)) return rce;
        staged.park();
    } else if (e_ == hipSuccess) e_ = staged.wait();
    if (e_ != hipSuccess) return hip_fail(e_, "upload of the marginalisation problems");
    s->d_dpool = (double *)s->d_input; s->d_hdr = (MargHdr *)((char *)s->d_input + lay.o_hdr); s->d_ipool = (int *)((char *)s->d_input + lay.o_int);
    return TCV_OK;
}

int tcv_marg_attach(tcv_batch *b, tcv_problem *const *marg_problems, double *const *const *marg_drop, const int *marg_num_drop) {
    MargState *s = new MargState();
    b->marg.reset(s);
    s->win.resize(b->in.n);
    for (int w = 0; w < b->in.n; w++)
        if (marg_problems[w] && (!marg_drop || !marg_drop[w])) { set_error("marginalisation problem without a drop list"); return TCV_ERR_INVALID; }
    const MargSwitches sw = MargSwitches::for_attach();
    MargPools P(b->in.n, tcv::host_threads(std::max(1, std::min(b->in.n <= 16 ? b->in.n : b->in.n / 8, 16))));      // (inside tcv_batch_create's HostOp; a lock-step frame's handful of windows: one each)
    if (int rc = marg_pack_windows(b, marg_problems, marg_drop, marg_num_drop, sw, s, P)) return rc;
    std::vector<MargHdr> hdrs(b->in.n);
    size_t lds_bytes = 0;
    if (int rc = marg_concat(s, P, hdrs, lds_bytes)) return rc;
    const MargBlobLayout lay(P.db[P.nth], P.ib[P.nth], hdrs.size());
    // (released at every exit; once the asynchronous upload has been issued the stream is drained first: the pinned buffer goes back to a
    // pool another host thread takes from)
    tcv::StagedTransfer staged(tcv::util_stream(), lay.bytes);
    if (!staged.host) { set_error("hipHostMalloc (upload staging) failed"); return TCV_ERR_HIP; }
    marg_fill_staging((char *)staged.host, lay, P, hdrs);
    if (int rc = marg_launch_shape(b, sw, lds_bytes, s)) return rc;
    if (int rc = marg_upload(b, s, staged, lay)) return rc;
    if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) return TCV_ERR_HIP;
    return TCV_OK;
}

int tcv_marg_run(tcv_batch *b, void *stream) {
    MargState *s = marg_of(b);
    if (!s) { set_error("batch was created without marginalisation problems"); return TCV_ERR_INVALID; }
    const MargSwitches sw = MargSwitches::for_run();
    MargArgs a;
    std::memset(&a, 0, sizeof a);
    a.hdr = s->d_hdr; a.ipool = s->d_ipool; a.dpool = s->d_dpool; a.solve_state = b->mem.d_state; a.out = s->d_out;
    a.out_status = s->d_status; a.scratch = s->d_scratch; a.nwin = b->in.n; a.state_stride = b->in.state_stride;
    a.use_solved_state = b->last.solved ? 1 : 0;
    a.solve_dpool = b->mem.d_dpool; a.solve_win = (const void *)b->mem.d_win;
    a.solve_sqrt = (b->last.solved && b->last.sqrt_out_valid && !sw.own_sqrt) ? b->mem.d_sqrt_out : nullptr;
    a.eig_mm = sw.eig_mm ? 1 : 0;
    a.eig_flags = sw.eig_flags;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipEventRecord(s->ev0, st)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    if (int rc = tcv_launch_marg(&a, s->grid, s->nt, s->lds_bytes, st)) return rc;
    if ((e = hipEventRecord(s->ev1, st)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    // what consumers of device-resident priors on other streams (and host readers) wait for: tcv_batch_get_priors_device_async hands the
    // results out while this kernel may still be running
    if (s->out_blob) {
        if (!s->out_blob->ready && hipEventCreateWithFlags(&s->out_blob->ready, hipEventDisableTiming) != hipSuccess) s->out_blob->ready = nullptr;
        if (s->out_blob->ready && (e = hipEventRecord(s->out_blob->ready, st)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    }
    s->ran = true;
    s->h_valid = false;
    s->status_prefetched = false;
    return TCV_OK;
}

// the statuses on their way to the host behind the marginalisation kernel (tcv_batch_get_priors_device_async): whoever asks later, after
// waiting for the batch, finds them in pinned memory instead of paying a blocking copy
int tcv_marg_status_prefetch(tcv_batch *b, void *stream) {
    MargState *s = marg_of(b);
    if (!s || !s->ran) return TCV_OK;
    if (!s->h_status_pre) s->h_status_pre = (int *)tcv::host_staging_acquire(sizeof(int) * 2 * (size_t)b->in.n);
    if (!s->h_status_pre) return TCV_OK;      // (the blocking copy later)
    const hipError_t e = hipMemcpyAsync(s->h_status_pre, s->d_status, sizeof(int) * 2 * (size_t)b->in.n, hipMemcpyDeviceToHost, (hipStream_t)stream);
    s->status_prefetched = e == hipSuccess;
    return TCV_OK;
}

int tcv_marg_layout_n(const tcv_batch *b, int window) {
    const MargState *s = marg_of(b);
    if (!s || window < 0 || window >= (int)s->win.size() || s->win[window].hdr.nblk == 0) return -1;
    return s->win[window].hdr.n;
}
bool tcv_marg_has_problem(const tcv_batch *b, int window) {
    const MargState *s = marg_of(b);
    return s && window >= 0 && window < b->in.n && (s->win[window].hdr.nblk != 0 || s->win[window].empty_keep);
}
int tcv_marg_sqrt_source(const tcv_batch *b, int window) {
    const MargState *s = marg_of(b);
    return (s && window >= 0 && window < b->in.n) ? s->win[window].hdr.sqrt_src : -1;
}

// one D2H copy of every window's result block and status instead of one copy per tcv_batch_get_prior call, into a pinned buffer.
// compact: J0, r0 and the linearisation point only (a strided copy of the first MARG_OUT_COMPACT doubles of every block); the priors
// handed out afterwards carry no A', b'.
int tcv_marg_download(tcv_batch *b, int compact) {
    MargState *s = marg_of(b);
    if (!s || !s->ran) { set_error("no marginalisation result"); return TCV_ERR_INVALID; }
    const size_t stride = compact ? (size_t)MARG_OUT_COMPACT : (size_t)MARG_OUT_STRIDE;
    if (s->h_out && s->h_stride != stride) { tcv::host_staging_release(s->h_out); s->h_out = nullptr; }
    const size_t out_bytes = sizeof(double) * stride * b->in.n;      // the status of every window rides behind the blocks in the same pinned buffer
    if (!s->h_out) s->h_out = (double *)tcv::host_staging_acquire(out_bytes + sizeof(int) * b->in.n);
    if (!s->h_out) { set_error("hipHostMalloc (download staging) failed"); return TCV_ERR_HIP; }
    s->h_stride = stride;
    s->h_status.resize(b->in.n);
    hipStream_t ust = tcv::util_stream();      // (h_out is pinned: asynchronous copies on the calling thread's own stream, one wait)
    hipError_t e = compact ? hipMemcpy2DAsync(s->h_out, sizeof(double) * stride, s->d_out, sizeof(double) * MARG_OUT_STRIDE, sizeof(double) * stride, b->in.n, hipMemcpyDeviceToHost, ust)
                           : hipMemcpyAsync(s->h_out, s->d_out, out_bytes, hipMemcpyDeviceToHost, ust);
    if (e == hipSuccess) e = hipMemcpyAsync((char *)s->h_out + out_bytes, s->d_status, sizeof(int) * b->in.n, hipMemcpyDeviceToHost, ust);
    const hipError_t ew = tcv::stream_wait(ust);      // (whatever was issued is drained before anybody touches h_out again)
    if (e == hipSuccess) e = ew;
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy D2H");
    std::memcpy(s->h_status.data(), (char *)s->h_out + out_bytes, sizeof(int) * b->in.n);
    s->h_valid = true;
    return TCV_OK;
}

// elapsed time of the last marginalisation launch (called from tcv_batch_synchronize)
void tcv_marg_elapsed(tcv_batch *b) {
    MargState *s = marg_of(b);
    if (s && s->ran) (void)hipEventElapsedTime(&b->last.marg_ms, s->ev0, s->ev1);
}

// per-window status of the last marginalisation: 0 ok, 1 an eigen-solver hit its sweep cap, 2 the tridiagonal eigen-solver's
// self-check failed and the cyclic-Jacobi safety net produced the result, < 0 not run
extern "C" int tcv_batch_marg_status(tcv_batch *b, int *out, int n) {
    MargState *s = b ? marg_of(b) : nullptr;
    if (!s || !s->ran || !out || n > b->in.n) { set_error("no marginalisation result"); return TCV_ERR_INVALID; }
    if (int rc = b->settle()) return rc;
    std::vector<int> st(2 * (size_t)b->in.n);
    if (s->status_prefetched) std::memcpy(st.data(), s->h_status_pre, sizeof(int) * st.size());      // (came down behind the kernel; the wait above covers it)
    else if (int rc = tcv::staged_download(st.data(), s->d_status, sizeof(int) * st.size(), "download of the marginalisation status")) return rc;
    for (int w = 0; w < n; w++)      // -2: a NaN in the result; a marginalisation that keeps nothing has nothing to run: 0
        out[w] = s->win[w].empty_keep ? 0 : ((st[w] == 0 && st[b->in.n + w] < 0 && s->win[w].hdr.nblk != 0) ? -2 : st[w]);
    return TCV_OK;
}

// kernel status of a window: TCV_OK, or the error it stands for
static int marg_status_error(int status) {
    if (status < 0) { set_error("marginalisation kernel did not complete for this window"); return TCV_ERR_NUMERIC; }
    // status 1: an eigen-solver ran into its sweep cap -- the decomposition is not converged and the prior would silently degrade every
    // later window (the reference's SelfAdjointEigenSolver has no such exit); status 2 (safety net took over) is a valid result
    if (status == 1) { set_error("marginalisation: eigen-decomposition did not converge (sweep cap)"); return TCV_ERR_NUMERIC; }
    return TCV_OK;
}
// host-side layout of the prior a window's marginalisation makes (no numbers yet): kept blocks' sizes, columns, offsets in x0, addresses
static tcv_prior *prior_layout(const MargWindow &mw) {
    tcv_prior *pr = new tcv_prior();
    pr->m = mw.m_total; pr->n = mw.hdr.n;     // the reference's m counts every marginalised dim (marginalization_factor.cpp:176-186)
    int xo = 0;
    for (size_t k = 0; k < mw.keep_block.size(); k++) {
        pr->size.push_back(mw.keep_size[k]);
        pr->idx.push_back(mw.keep_idx[k] - mw.hdr.m);      // (hdr.m: dropped dims that went through the eigen step)
        pr->xoff.push_back(xo);
        xo += mw.keep_size[k];
        pr->addr.push_back(mw.keep_addr[k]);
    }
    pr->xsize = xo;
    return pr;
}

// TCV_DEBUG: the diagnostic slots of a window's result block (tcv_marg.h MARG_DIAG_*) on stderr
static void marg_debug_dump(const double *o, int window, int m, int n, int status) {
    fprintf(stderr, "[tcv] marg window %d: m=%d n=%d jacobi sweeps %g / %g status %d\n", window, m, n, o[MARG_DIAG_SWEEPS_MM], o[MARG_DIAG_SWEEPS_RR], status);
    const char *nm[12] = {"load", "prior", "imu", "proj", "eig_mm", "Z", "schur", "eig_rr", "out", "j_angle|chol_mm", "j_cols|barrier", "j_rows|subst_mm"};      // (9..11: Jacobi safety net, or the register Cholesky route of Amm)
    fprintf(stderr, "[tcv]   Amm: trace(Amm^-1) %.3e, of the unit-diagonal scaling %.3e\n", o[MARG_DIAG_AMM_TRACE], o[MARG_DIAG_AMM_TRACE + 1]);
    for (int i = 0; i < 12; i++) fprintf(stderr, "[tcv]   %-7s %12.0f cycles\n", nm[i], o[MARG_DIAG_PHASE + i]);
    const double *sub = o + MARG_DIAG_PROJ_SUB, *step = o + MARG_DIAG_TRIDIAG_STEP, *chk = o + MARG_DIAG_EIG_CHECK;
    fprintf(stderr, "[tcv]     proj, chunked block path: evaluation + chunk set-up %.0f | accumulation %.0f | landmark elimination %.0f cycles\n", sub[1], sub[2], sub[3]);
    const char *en[6] = {"tridiag", "bisect", "vectors", "mgs", "backtr", "check"};
    for (int i = 0; i < 6; i++) fprintf(stderr, "[tcv]     eig_rr.%-8s %10.0f cycles\n", en[i], o[MARG_DIAG_EIG_PHASE + i]);
    fprintf(stderr, "[tcv]     tridiag steps (wave 0): part 1 %.0f | barrier %.0f | update m > 40 %.0f, m > 16 %.0f, m <= 16 %.0f | barrier %.0f cycles\n", step[0], step[1], step[2], step[3], step[4], step[5]);
    fprintf(stderr, "[tcv]   tridiag check: dev %.3e sum(lam) %.10e trace %.10e |T| %.3e lam_min %.3e lam_max %.3e\n", chk[0], chk[1], chk[2], chk[3], chk[4], chk[5]);
}

int tcv_marg_get_prior(tcv_batch *b, int window, tcv_prior **out) {
    MargState *s = marg_of(b);
    if (!s || !s->ran || window < 0 || window >= b->in.n) { set_error("no marginalisation result for this window"); return TCV_ERR_INVALID; }
    const MargWindow &mw = s->win[window];
    if (mw.empty_keep) { tcv_prior *pr = new tcv_prior(); pr->m = mw.m_total; pr->n = 0; *out = pr; return TCV_OK; }      // the reference's empty MarginalizationInfo
    if (mw.hdr.nblk == 0) { set_error("this window of the batch has no marginalisation problem"); return TCV_ERR_INVALID; }
    const int n = mw.hdr.n, m = mw.hdr.m;      // m: dropped dims that went through the eigen step (all of them unless block mode)
    std::vector<double> o(MARG_OUT_STRIDE);
    int status = -1;
    bool have_schur = true;
    if (s->h_valid) {
        std::copy(s->h_out + (size_t)window * s->h_stride, s->h_out + (size_t)(window + 1) * s->h_stride, o.begin());
        have_schur = s->h_stride == (size_t)MARG_OUT_STRIDE;
        status = s->h_status[window];
    } else {
        // one round trip: the window's result block and, behind it in the staging buffer, its status (they are not neighbours on the device)
        const size_t ob = sizeof(double) * MARG_OUT_STRIDE;
        tcv::StagedTransfer dl(tcv::util_stream(), ob + sizeof(int));
        if (!dl.host) { set_error("hipHostMalloc (download staging) failed"); return TCV_ERR_HIP; }
        dl.issued();
        hipError_t e = hipMemcpyAsync(dl.host, s->d_out + (size_t)window * MARG_OUT_STRIDE, ob, hipMemcpyDeviceToHost, dl.st);
        if (e == hipSuccess) e = hipMemcpyAsync((char *)dl.host + ob, s->d_status + window, sizeof(int), hipMemcpyDeviceToHost, dl.st);
        if (e == hipSuccess) e = dl.wait();
        if (e != hipSuccess) return hip_fail(e, "download of a marginalisation result");
        std::memcpy(o.data(), dl.host, ob); std::memcpy(&status, (char *)dl.host + ob, sizeof(int));
    }
    if (int rc = marg_status_error(status)) return rc;
    tcv_prior *pr = prior_layout(mw);
    for (size_t k = 0; k < mw.keep_block.size(); k++)
        for (int i = 0; i < mw.keep_size[k]; i++) pr->x0.push_back(o[MARG_OUT_X + mw.keep_goff[k] + i]);
    pr->J0.assign(o.begin() + MARG_OUT_J0, o.begin() + MARG_OUT_J0 + (size_t)n * n);
    pr->r0.assign(o.begin() + MARG_OUT_R0, o.begin() + MARG_OUT_R0 + n);
    if (have_schur) {
        pr->As.assign(o.begin() + MARG_OUT_AS, o.begin() + MARG_OUT_AS + (size_t)n * n);
        pr->bs.assign(o.begin() + MARG_OUT_BS, o.begin() + MARG_OUT_BS + n);
    }
    if (getenv("TCV_DEBUG")) marg_debug_dump(o.data(), window, m, n, status);
    for (double v : pr->J0) if (!(v == v)) { delete pr; set_error("NaN in marginalisation result"); return TCV_ERR_NUMERIC; }
    *out = pr;
    return TCV_OK;
}

// tcv_batch_get_priors_device: layout on the host, numbers left in the batch's result buffer (shared with the handles)
int tcv_marg_get_priors_device(tcv_batch *b, tcv_prior **out, int n, bool nowait) {
    MargState *s = marg_of(b);
    if (!s || !s->ran || n != b->in.n) { set_error("no marginalisation result (or n is not the batch size)"); return TCV_ERR_INVALID; }
    if (nowait && !(s->out_blob && s->out_blob->ready)) {      // (no event to order consumers by: wait as usual)
        nowait = false;
        if (int rcs = b->settle()) return rcs;
    }
    std::vector<int> st(2 * (size_t)n, 0);
    if (nowait) { for (int w = 0; w < n; w++) st[n + w] = -1; }      // status unknown here (tcv_batch_marg_status later), k0 read on the device
    else if (int rcd = tcv::staged_download(st.data(), s->d_status, sizeof(int) * st.size(), "hipMemcpy D2H (marginalisation status)")) return rcd;
    for (int w = 0; w < n; w++) out[w] = nullptr;
    int rc = TCV_OK;
    for (int w = 0; w < n && rc == TCV_OK; w++) {
        const MargWindow &mw = s->win[w];
        if (mw.empty_keep) { tcv_prior *pr = new tcv_prior(); pr->m = mw.m_total; pr->n = 0; out[w] = pr; continue; }      // empty prior: host-resident, nothing to splice
        if (mw.hdr.nblk == 0) continue;      // not marginalised: out[w] stays NULL
        const int status = st[w], k0 = st[n + w];
        if ((rc = marg_status_error(status)) != TCV_OK) break;
        if (k0 < 0 && !nowait) { set_error("NaN in marginalisation result"); rc = TCV_ERR_NUMERIC; break; }
        if ((int)mw.keep_block.size() > PRIOR_SPLICE_MAX_BLOCKS) { set_error("device-resident prior: too many kept blocks"); rc = TCV_ERR_TOO_LARGE; break; }
        tcv_prior *pr = prior_layout(mw);
        pr->x_goff.assign(mw.keep_goff.begin(), mw.keep_goff.begin() + mw.keep_block.size());
        pr->dev = s->out_blob; pr->d_block = s->d_out + (size_t)w * MARG_OUT_STRIDE; pr->k0 = k0; pr->host = false;
        pr->d_status = s->d_status + w; pr->d_k0 = s->d_status + n + w;
        out[w] = pr;
    }
    if (rc != TCV_OK) for (int w = 0; w < n; w++) if (out[w]) { delete out[w]; out[w] = nullptr; }
    return rc;
}
