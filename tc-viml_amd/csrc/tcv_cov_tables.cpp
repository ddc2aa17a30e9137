// The side tables of the marginal covariance (layouts: tcv_cov.h; declared in tcv_host.h): the request resolver, the owner lists of the
// reduced camera system S, the landmark slot tables and the request tables.  Pure host code -- functions of a problem, its packed window and
// the plan header, with no device call; the buffers they go into and the C-ABI are tcv_cov_host.cpp.
#include <algorithm>
#include <map>

#include "../../include/tcv_covariance.h"
#include "tcv_cov.h"
#include "tcv_host.h"

namespace tcv {
namespace {
int block_width(const ParamBlock &pb) { return pb.kind == KIND_POSE ? 6 : pb.size; }
// offsets of the J region's parts behind the IMU factors (tcv_cov.h): point factors, line factors, 1 / H_ll, the slots of h_l
struct JRegion {
    int proj, line, hll, h;
    explicit JRegion(const PlanHdr &H) : proj(COV_J_IMU * H.n_imu), line(proj + COV_J_PROJ * H.n_proj), hll(line + COV_J_LINE * H.n_line), h(hll + 2 * H.nland) {}
};
const int PROJ_COL0[4] = {0, 6, 12, 19};      // first column of pose_i, pose_j, extrinsic, td in a point factor's 2 x 20 Jacobian
// the block pairs of S with their items, keyed and therefore emitted by (ta, tb)
struct Pairs {
    struct Pair { int wa = 0, wb = 0, pca = -1, pcb = -1; std::vector<int> items; };
    const tcv_problem &p;
    const BlockMap &map;
    std::map<std::pair<int, int>, Pair> pairs;
    bool repeated = false;      // a factor names one block twice
    // one item of the pair (block A, block B): offsets of the two column blocks in the J region
    void add(int A, int offA, int B, int offB, int rows, int stride, int sc) {
        int ta = map.toff(A), tb = map.toff(B);
        if (ta < 0 || tb < 0) return;
        if (A == B && offA != offB) repeated = true;
        if (ta < tb) { std::swap(ta, tb); std::swap(A, B); std::swap(offA, offB); }
        Pair &q = pairs[{ta, tb}];
        q.wa = block_width(p.blocks[A]); q.wb = block_width(p.blocks[B]);
        const int it[4] = {offA, offB, rows << 16 | stride, sc};
        q.items.insert(q.items.end(), it, it + 4);
    }
};
// phase 1: the items of the IMU, point and line factors, in that order; refuses a constant inverse depth
int factor_items(const tcv_problem &p, const Packed &pk, const JRegion &R, Pairs &P) {
    for (size_t f = 0; f < p.imu.size(); f++) {
        static const int col0[4] = {0, 6, 15, 21};
        for (int x = 0; x < 4; x++) for (int y = 0; y <= x; y++)
            P.add(p.imu[f].b[x], (int)f * COV_J_IMU + col0[x], p.imu[f].b[y], (int)f * COV_J_IMU + col0[y], 15, 30, -1);
    }
    for (size_t k = 0; k < pk.proj_order.size(); k++) {
        const ProjFac &f = p.proj[pk.proj_order[k]];
        const int bl[4] = {f.b[0], f.b[1], f.b[2], f.btd}, base = R.proj + (int)k * COV_J_PROJ;
        for (int x = 0; x < 4; x++) for (int y = 0; y <= x; y++)
            if (bl[x] >= 0 && bl[y] >= 0) P.add(bl[x], base + PROJ_COL0[x], bl[y], base + PROJ_COL0[y], 2, 20, -1);
        if (P.map.lm_of(f.b[3]) < 0 || p.blocks[f.b[3]].constant) { set_error("covariance: a constant inverse depth is not supported"); return TCV_ERR_UNSUPPORTED; }
    }
    for (size_t k = 0; k < p.line.size(); k++) P.add(p.line[k].b, R.line + (int)k * COV_J_LINE, p.line[k].b, R.line + (int)k * COV_J_LINE, 2, 6, -1);
    return TCV_OK;
}
// phase 3: the prior -- every pair of its variable blocks
void prior_pairs(const tcv_problem &p, const PlanHdr &H, Pairs &P) {
    if (H.prior_n <= 0 || p.prior.empty()) return;
    const tcv_prior *pr = p.prior[0].prior;
    const std::vector<int> &pb = p.prior[0].b;
    for (size_t x = 0; x < pb.size(); x++) for (size_t y = 0; y < pb.size(); y++) {
        const int ta = P.map.toff(pb[x]), tb = P.map.toff(pb[y]);
        if (ta < 0 || tb < 0 || ta < tb) continue;
        Pairs::Pair &q = P.pairs[{ta, tb}];
        q.wa = block_width(p.blocks[pb[x]]); q.wb = block_width(p.blocks[pb[y]]);
        q.pca = pr->idx[x]; q.pcb = pr->idx[y];
    }
}
}  // namespace

int cov_resolve(const tcv_problem &p, int kind, int index, int *blk, int *width) {
    auto frame = [&](const std::vector<int> &tab, const char *what) -> int {
        const int n = (int)tab.size();
        if (n == 0) { set_error(std::string("covariance: the window lacks a requested block: no frame table for ") + what + " (tcv_problem_set_frames)"); return -1; }
        const int i = index < 0 ? index + n : index;
        if (i < 0 || i >= n) { set_error(std::string("covariance: ") + what + " index out of range"); return -1; }
        if (tab[i] < 0) { set_error(std::string("covariance: the window lacks a requested block: ") + what + " of that frame"); return -1; }
        return tab[i];
    };
    auto single = [&](int b, const char *what) -> int {
        if (index != 0 && index != -1) { set_error(std::string("covariance: ") + what + " index out of range (0)"); return -1; }
        if (b < 0) { set_error(std::string("covariance: the window lacks a requested block: ") + what); return -1; }
        return b;
    };
    int b = -1;
    switch (kind) {
    case TCV_COV_POSE: b = frame(p.frame_pose, "pose"); break;
    case TCV_COV_SPEED_BIAS: b = frame(p.frame_sb, "speed-bias"); break;
    case TCV_COV_EXTRINSIC: b = single(p.proj.empty() ? -1 : p.proj[0].b[2], "extrinsic (no point factors)"); break;
    case TCV_COV_TD: b = single(p.proj.empty() ? -1 : p.proj[0].btd, "td (no para_Td)"); break;
    case TCV_COV_RELO_POSE: b = single(p.relo_block, "relocalisation pose"); break;
    case TCV_COV_LANDMARK: set_error("covariance: landmark (inverse depth) blocks are not supported: camera-side blocks only"); return TCV_ERR_UNSUPPORTED;
    default: set_error("covariance: unknown block kind"); return TCV_ERR_INVALID;
    }
    if (b < 0) return TCV_ERR_INVALID;
    if (blk) *blk = b;
    if (width) *width = block_width(p.blocks[b]);
    return TCV_OK;
}
CovLmSlots cov_landmark_slots(const tcv_problem &p, const Packed &pk, const PlanHdr &H) {
    const BlockMap map(p, pk);
    const JRegion R(H);
    std::vector<std::vector<int>> lm_fac(H.nland);
    for (size_t k = 0; k < pk.proj_order.size(); k++) lm_fac[map.lm_of(p.proj[pk.proj_order[k]].b[3])].push_back((int)k);
    CovLmSlots S;
    for (int l = 0; l < H.nland; l++) {
        const size_t s0 = S.blk.size();
        for (int k : lm_fac[l]) {
            const ProjFac &f = p.proj[pk.proj_order[k]];
            const int bl[4] = {f.b[0], f.b[1], f.b[2], f.btd}, base = R.proj + k * COV_J_PROJ;
            for (int x = 0; x < 4; x++) {
                if (bl[x] < 0 || map.toff(bl[x]) < 0) continue;
                size_t s = std::find(S.blk.begin() + s0, S.blk.end(), bl[x]) - S.blk.begin();
                if (s == S.blk.size()) { S.blk.push_back(bl[x]); S.items.emplace_back(); }
                S.items[s].push_back(base + PROJ_COL0[x]); S.items[s].push_back(base + 18);
            }
            S.lmfac.push_back(k);
        }
        S.lmptr.push_back((int)S.lmfac.size());
        for (size_t s = s0; s < S.blk.size(); s++) S.off.push_back(R.h + COV_SLOT * (int)s);
        S.sptr.push_back((int)S.blk.size());
    }
    S.jdoubles = R.h + COV_SLOT * (int)S.blk.size();
    return S;
}
int cov_owner_lists(const tcv_problem &p, const Packed &pk, const PlanHdr &H, std::vector<int> &out, int *jdoubles) {
    const BlockMap map(p, pk);
    const JRegion R(H);
    Pairs P{p, map};
    if (int rc = factor_items(p, pk, R, P)) return rc;
    // phase 2, the landmarks: the slots of h_l with their owner lists, and the pair items
    const CovLmSlots S = cov_landmark_slots(p, pk, H);
    std::vector<int> hslot, hitem;
    for (int l = 0; l < H.nland; l++) {
        const int s0 = S.sptr[l], s1 = S.sptr[l + 1];
        for (int s = s0; s < s1; s++) {
            const int rec[CT_HSLOT] = {S.off[s], block_width(p.blocks[S.blk[s]]), (int)hitem.size() / CT_HITEM, (int)(hitem.size() + S.items[s].size()) / CT_HITEM};
            hslot.insert(hslot.end(), rec, rec + CT_HSLOT);
            hitem.insert(hitem.end(), S.items[s].begin(), S.items[s].end());
        }
        for (int x = s0; x < s1; x++) for (int y = s0; y <= x; y++) P.add(S.blk[x], S.off[x], S.blk[y], S.off[y], 1, 0, R.hll + 2 * l);
    }
    if (P.repeated) { set_error("covariance: a factor that names one parameter block twice is not supported"); return TCV_ERR_UNSUPPORTED; }
    prior_pairs(p, H, P);
    // phase 4: header | pairs | items | hslot | hitem | lmptr | lmfac
    out.assign(CT_HDR, 0);
    out[CT_NPAIR] = (int)P.pairs.size(); out[CT_OPAIR] = CT_HDR;
    std::vector<int> items;
    for (auto &kv : P.pairs) {
        const Pairs::Pair &q = kv.second;
        const int rec[CT_PAIR] = {kv.first.first, kv.first.second, q.wa, q.wb, (int)items.size() / CT_ITEM, (int)(items.size() + q.items.size()) / CT_ITEM, q.pca, q.pcb};
        out.insert(out.end(), rec, rec + CT_PAIR);
        items.insert(items.end(), q.items.begin(), q.items.end());
    }
    auto put = [&](int slot, const std::vector<int> &v) { out[slot] = (int)out.size(); out.insert(out.end(), v.begin(), v.end()); };
    put(CT_OITEM, items);
    out[CT_NHSLOT] = (int)hslot.size() / CT_HSLOT;
    put(CT_OHSLOT, hslot); put(CT_OHITEM, hitem); put(CT_OLMPTR, S.lmptr); put(CT_OLMFAC, S.lmfac);
    out[CT_JPROJ] = R.proj; out[CT_JLINE] = R.line; out[CT_JHLL] = R.hll; out[CT_JDOUBLES] = S.jdoubles;
    *jdoubles = S.jdoubles;
    return TCV_OK;
}
std::vector<int> cov_slot_table(const tcv_problem &p, const Packed &pk, const CovLmSlots &S) {
    const BlockMap map(p, pk);
    std::vector<int> lt(1, 0), lslot;
    for (size_t l = 0; l + 1 < S.sptr.size(); l++) {
        std::vector<std::pair<int, int>> by_row;
        for (int s = S.sptr[l]; s < S.sptr[l + 1]; s++) by_row.push_back({map.toff(S.blk[s]), s});
        std::sort(by_row.begin(), by_row.end());
        for (auto &r : by_row) { const int rec[LT_SLOT] = {r.first, S.off[r.second], block_width(p.blocks[S.blk[r.second]])}; lslot.insert(lslot.end(), rec, rec + LT_SLOT); }
        lt.push_back((int)lslot.size() / LT_SLOT);
    }
    lt.insert(lt.end(), lslot.begin(), lslot.end());
    return lt;
}
int cov_request_tables(const tcv_batch *b, const tcv_covariance_block *blocks, int n_req, std::vector<int> &rq, std::vector<int> &rows, std::vector<int> &cols) {
    const int n = b->in.n, stride = cov_rq_stride(n_req);
    rq.assign((size_t)n * stride, 0); rows.assign(n_req, 0); cols.assign(n_req, 0);
    for (int w = 0; w < n; w++) {
        const tcv_problem &p = *b->in.problems[w];
        const BlockMap map(p, b->in.packed[w]);
        int *q = rq.data() + (size_t)w * stride, m = 0;
        std::map<int, int> col_of;      // first tangent index of a block -> its first solved column
        auto column = [&](int blk, int width) -> int {
            const int t = map.toff(blk);
            if (t < 0) return -1;
            auto it = col_of.find(t);
            if (it != col_of.end()) return it->second;
            for (int j = 0; j < width; j++) q[RQ_COL + m + j] = t + j;
            col_of[t] = m; m += width;
            return m - width;
        };
        for (int k = 0; k < n_req; k++) {
            int bi = -1, bj = -1, wi = 0, wj = 0;
            if (int rc = cov_resolve(p, blocks[k].kind_i, blocks[k].index_i, &bi, &wi)) return rc;
            if (int rc = cov_resolve(p, blocks[k].kind_j, blocks[k].index_j, &bj, &wj)) return rc;
            if (map.cam_of(bi) < 0 || map.cam_of(bj) < 0) { set_error("covariance: a requested block is not on the camera side of the window"); return TCV_ERR_INVALID; }
            if (w > 0 && (wi != rows[k] || wj != cols[k])) { set_error("covariance: a requested block has different sizes in two windows"); return TCV_ERR_INVALID; }
            rows[k] = wi; cols[k] = wj;
            int *r = q + RQ_REQ + 4 * k;
            r[0] = column(bi, wi); r[1] = wi; r[2] = column(bj, wj); r[3] = wj;
        }
        q[RQ_M] = m; q[RQ_NREQ] = n_req;
    }
    return TCV_OK;
}
}  // namespace tcv
