// mgmc_panel.hip -- the QoI panel (mgmc_panel.hpp): its two launches and the mgmc_qoi_panel_* entry points.
// A translation unit of its own, so that its kernels form a code object of their own: a handle that never installs
// a panel loads exactly the device code it loaded before the panel existed.
#include "mgmc_internal.hpp"
#include "mgmc_panel.hpp"

namespace mgmc_host {
// ---- QoI panel (mgmc_panel.hpp): the K dots of every chain's level-0 state, then the record ----
// ctl (recording, the cycle's op): only on a recorded cycle, then the series, the moments, the autocovariance and
// the counters; ctl == nullptr (mgmc_qoi_panel_eval): the dots into qp_out, nothing else.  (MGMC_POISON: the op's
// LDS fill precedes k_panel_dots, which uses no LDS, so k_panel_record still starts on NaN-filled LDS.)
void launch_panel(mgmc_handle* h, uint64_t* ctl, hipStream_t s) {
    const Level& lv = h->levels[0];
    const int nch = h->nchains;
    hipLaunchKernelGGL(k_panel_dots, dim3(h->qp_nwork, nch), dim3(64), 0, s, lv.L, (const PanelWork*)h->qp_work,
                       (const long long*)h->qp_ent_off, (const double*)h->qp_ent_val, (const double*)h->qp_dense_val,
                       (const double*)lv.x, (long long)lv.L.nstore, h->qp_part, h->qp_nslot, (const uint64_t*)ctl);
    PanelRecordArgs a;
    a.col = h->qp_col;
    a.part = h->qp_part;
    a.K = h->qp_K;
    a.nslot = h->qp_nslot;
    a.ctl = ctl;
    a.out = ctl ? nullptr : h->qp_out;
    a.series = h->qp_series;
    a.mom = h->qp_mom;
    a.ring = h->qp_ring;
    a.S = h->qp_S;
    hipLaunchKernelGGL(k_panel_record, dim3(nch), dim3(QP_NT), 0, s, a);
}
}  // namespace mgmc_host

extern "C" {

// ---------------- QoI panel: K functionals per cycle and their joint statistics (mgmc_panel.hpp) ----------------

extern "C++" {
namespace {
// device buffers of a panel being installed / of a record being enabled: freed unless the handle took them
struct PanelAllocs {
    std::vector<void*> p;
    bool keep = false;
    ~PanelAllocs() {
        if (!keep)
            for (void* q : p) hipFree(q);
    }
    template <class T>
    bool get(T** out, size_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        p.push_back(q);
        *out = (T*)q;
        return true;
    }
};

struct PanelRecordBufs {
    uint64_t* ctl = nullptr;
    double *series = nullptr, *mom = nullptr, *ring = nullptr, *S = nullptr;
};

size_t panel_mom_doubles(int K) { return 1 + (size_t)K + (size_t)K * K; }

bool panel_record_alloc(const mgmc_handle* h, PanelAllocs& al, int K, int window, uint64_t cap, PanelRecordBufs* b) {
    const size_t nch = (size_t)h->nchains;
    return al.get(&b->ctl, nch * QP_CTL_WORDS) && al.get(&b->series, nch * cap * K) &&
           al.get(&b->mom, nch * panel_mom_doubles(K)) && al.get(&b->ring, nch * window * K) &&
           al.get(&b->S, nch * K * window);
}

void panel_free_record(mgmc_handle* h) {
    if (h->qp_ctl) hipFree(h->qp_ctl);
    if (h->qp_series) hipFree(h->qp_series);
    if (h->qp_mom) hipFree(h->qp_mom);
    if (h->qp_ring) hipFree(h->qp_ring);
    if (h->qp_S) hipFree(h->qp_S);
    h->qp_ctl = nullptr;
    h->qp_series = h->qp_mom = h->qp_ring = h->qp_S = nullptr;
    h->qp_stride = h->qp_window = 0;
    h->qp_cap = 0;
}

void panel_take_record(mgmc_handle* h, const PanelRecordBufs& b, int window, uint64_t cap) {
    h->qp_ctl = b.ctl, h->qp_series = b.series, h->qp_mom = b.mom, h->qp_ring = b.ring, h->qp_S = b.S;
    h->qp_window = window;
    h->qp_cap = cap;
    const size_t nch = (size_t)h->nchains;
    poison_fill(h, b.series, nch * cap * h->qp_K * sizeof(double));
    poison_fill(h, b.ring, nch * window * h->qp_K * sizeof(double));
}

// zero the moments, the autocovariance and the counters, set the stride (capacity and window stay)
int panel_zero(mgmc_handle* h, int stride) {
    const size_t nch = (size_t)h->nchains;
    std::vector<uint64_t> ctl0(nch * QP_CTL_WORDS, 0);
    for (size_t c = 0; c < nch; ++c) {
        ctl0[c * QP_CTL_WORDS + 2] = (uint64_t)stride;
        ctl0[c * QP_CTL_WORDS + 3] = h->qp_cap;
        ctl0[c * QP_CTL_WORDS + 4] = (uint64_t)h->qp_window;
    }
    HIPCHK(h, hipMemsetAsync(h->qp_mom, 0, nch * panel_mom_doubles(h->qp_K) * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->qp_S, 0, nch * h->qp_K * h->qp_window * sizeof(double), h->stream));
    HIPCHK(h, hipMemcpyAsync(h->qp_ctl, ctl0.data(), ctl0.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (ctl0 is on this stack)
    h->qp_stride = stride;
    return MGMC_OK;
}

void panel_free(mgmc_handle* h) {
    for (void* p : h->qp_allocs) hipFree(p);
    h->qp_allocs.clear();
    h->qp_K = h->qp_nwork = h->qp_nslot = 0;
    h->qp_work = nullptr;
    h->qp_col = nullptr;
    h->qp_ent_off = nullptr;
    h->qp_ent_val = h->qp_dense_val = h->qp_part = h->qp_out = nullptr;
}

// chain 0's ctl[0], ctl[1] of an enabled handle (every chain's copy holds the same; waits for the stream)
int panel_counters(const mgmc_handle* h, uint64_t out[2]) {
    if (hipSetDevice(h->device) != hipSuccess ||
        hipMemcpyAsync(out, h->qp_ctl, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(nullptr, MGMC_E_HIP, "QoI panel: reading the counters failed");
    return MGMC_OK;
}
}  // namespace
}  // extern "C++"

int mgmc_qoi_panel_set(mgmc_handle* h, int K, const int64_t* colptr, const int64_t* rows, const double* vals) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (K < 0 || K > QP_MAX_K) return fail(h, MGMC_E_INVALID, "QoI panel: K must be in [0, 64]");
    if (K > 0 && (!colptr || !rows || !vals)) return fail(h, MGMC_E_INVALID, "QoI panel: null argument");
    const Level& lv = h->levels[0];
    const int64_t N = (int64_t)lv.spec.ndof;
    // ---- validate everything before the handle is touched ----
    if (K > 0 && colptr[0] != 0) return fail(h, MGMC_E_INVALID, "QoI panel: colptr[0] must be 0");
    for (int k = 0; k < K; ++k) {
        if (colptr[k + 1] < colptr[k]) return fail(h, MGMC_E_INVALID, "QoI panel: colptr must not decrease");
        if (colptr[k + 1] == colptr[k])
            return fail(h, MGMC_E_INVALID, "QoI panel: column " + std::to_string(k) + " is empty");
        if (colptr[k + 1] - colptr[k] > N)
            return fail(h, MGMC_E_INVALID, "QoI panel: column " + std::to_string(k) + " lists more rows than vertices");
        for (int64_t e = colptr[k]; e < colptr[k + 1]; ++e) {
            if (rows[e] < 0 || rows[e] >= N || (e > colptr[k] && rows[e] <= rows[e - 1]))
                return fail(h, MGMC_E_INVALID, "QoI panel: rows must be strictly ascending vertex indices (column " +
                                                   std::to_string(k) + ")");
            if (!std::isfinite(vals[e]))
                return fail(h, MGMC_E_INVALID, "QoI panel: non-finite value in column " + std::to_string(k));
        }
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const bool recording = h->qp_ctl != nullptr;
    if (K == 0) {  // remove (a recording ends with its panel)
        if (recording) destroy_graphs(h);
        panel_free_record(h);
        panel_free(h);
        if (!recording) return MGMC_OK;
        sync_fieldstats_op(h);
        return build_graphs(h);
    }
    // ---- the host side of the device arrays ----
    const int64_t nxi = lv.L.nx - 1, nyi = lv.L.ny - 1;
    std::vector<PanelColumn> col((size_t)K);
    std::vector<PanelWork> work;
    std::vector<long long> ent_off;
    std::vector<double> ent_val, dense_val;
    std::vector<int> dense_cols;
    int nslot = 0;
    const int nblk_dense = (int)((N + QP_BLK - 1) / QP_BLK);
    std::vector<long long> dense_src((size_t)K, 0);
    std::vector<int> dense_cflag((size_t)K, 0);
    for (int k = 0; k < K; ++k) {
        const int64_t n = colptr[k + 1] - colptr[k];
        col[(size_t)k].slot0 = nslot;
        col[(size_t)k].nblk = (int)((n + QP_BLK - 1) / QP_BLK);
        nslot += col[(size_t)k].nblk;
        if (n == N) {  // every vertex listed (strictly ascending in [0, N)): a dense column
            dense_cols.push_back(k);
            const double* v = vals + colptr[k];
            bool same = true;
            for (int64_t e = 1; e < n && same; ++e) same = memcmp(v + e, v, sizeof(double)) == 0;
            dense_cflag[(size_t)k] = same ? 1 : 0;
            if (!same) {
                dense_src[(size_t)k] = (long long)dense_val.size();
                dense_val.insert(dense_val.end(), v, v + n);
            }
        }
    }
    for (size_t g0 = 0; g0 < dense_cols.size(); g0 += QP_G) {  // the dense groups first: the long wavefronts
        const int ncol = (int)std::min<size_t>(QP_G, dense_cols.size() - g0);
        for (int b = 0; b < nblk_dense; ++b) {
            PanelWork w;
            memset(&w, 0, sizeof(w));
            w.e0 = (long long)b * QP_BLK;
            w.cnt = (int)std::min<int64_t>(QP_BLK, N - w.e0);
            w.ncol = ncol;
            w.dense = 1;
            for (int g = 0; g < ncol; ++g) {
                const int k = dense_cols[g0 + (size_t)g];
                w.src[g] = dense_src[(size_t)k] + w.e0;
                w.slot[g] = col[(size_t)k].slot0 + b;
                w.cflag[g] = dense_cflag[(size_t)k];
                w.cval[g] = vals[colptr[k]];
            }
            work.push_back(w);
        }
    }
    for (int k = 0; k < K; ++k) {
        const int64_t n = colptr[k + 1] - colptr[k];
        if (n == N) continue;
        const long long ent0 = (long long)ent_off.size();
        for (int64_t e = colptr[k]; e < colptr[k + 1]; ++e) {
            const int i = (int)(rows[e] % nxi) + 1, j = (int)((rows[e] / nxi) % nyi) + 1;
            const int kk = lv.spec.dim == 3 ? (int)(rows[e] / (nxi * nyi)) + 1 : 0;
            ent_off.push_back(lv.L.at(i, j, kk));
            ent_val.push_back(vals[e]);
        }
        for (int b = 0; b < col[(size_t)k].nblk; ++b) {
            PanelWork w;
            memset(&w, 0, sizeof(w));
            w.e0 = (long long)b * QP_BLK;
            w.cnt = (int)std::min<int64_t>(QP_BLK, n - w.e0);
            w.ncol = 1;
            w.src[0] = ent0 + w.e0;
            w.slot[0] = col[(size_t)k].slot0 + b;
            work.push_back(w);
        }
    }
    // ---- the device side: the handle takes the new panel (and a recording its new buffers) only once all are there
    PanelAllocs al, alr;
    PanelWork* d_work = nullptr;
    PanelColumn* d_col = nullptr;
    long long* d_off = nullptr;
    double *d_val = nullptr, *d_dense = nullptr, *d_part = nullptr, *d_out = nullptr;
    const size_t nch = (size_t)h->nchains;
    PanelRecordBufs rb;
    if (!al.get(&d_work, work.size()) || !al.get(&d_col, (size_t)K) || !al.get(&d_off, ent_off.size()) ||
        !al.get(&d_val, ent_val.size()) || !al.get(&d_dense, dense_val.size()) || !al.get(&d_part, nch * nslot) ||
        !al.get(&d_out, nch * K) ||
        (recording && !panel_record_alloc(h, alr, K, h->qp_window, h->qp_cap, &rb)))
        return fail(h, MGMC_E_NOMEM, "device allocation failed (QoI panel)");
    HIPCHK(h, hipMemcpy(d_work, work.data(), work.size() * sizeof(PanelWork), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_col, col.data(), col.size() * sizeof(PanelColumn), hipMemcpyHostToDevice));
    if (!ent_off.empty()) {
        HIPCHK(h, hipMemcpy(d_off, ent_off.data(), ent_off.size() * sizeof(long long), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d_val, ent_val.data(), ent_val.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!dense_val.empty())
        HIPCHK(h, hipMemcpy(d_dense, dense_val.data(), dense_val.size() * sizeof(double), hipMemcpyHostToDevice));
    if (recording) destroy_graphs(h);  // (they hold the old panel's addresses)
    panel_free(h);
    al.keep = true;
    h->qp_allocs = al.p;
    h->qp_K = K;
    h->qp_nwork = (int)work.size();
    h->qp_nslot = nslot;
    h->qp_work = d_work, h->qp_col = d_col, h->qp_ent_off = d_off, h->qp_ent_val = d_val, h->qp_dense_val = d_dense;
    h->qp_part = d_part, h->qp_out = d_out;
    poison_fill(h, d_part, nch * nslot * sizeof(double));
    poison_fill(h, d_out, nch * K * sizeof(double));
    if (!recording) return MGMC_OK;
    // a new panel while recording: the records start again (same stride, window and capacity)
    const int stride = h->qp_stride, window = h->qp_window;
    const uint64_t cap = h->qp_cap;
    panel_free_record(h);
    alr.keep = true;
    panel_take_record(h, rb, window, cap);
    int rc = panel_zero(h, stride);
    if (rc == MGMC_OK) rc = build_graphs(h);
    if (rc != MGMC_OK) {  // the new panel stays installed, not recording: back to the cycle without the op
        const std::string err = h->last_error;
        destroy_graphs(h);
        panel_free_record(h);
        sync_fieldstats_op(h);
        (void)build_graphs(h);
        return fail(h, rc, err);
    }
    return MGMC_OK;
}

int mgmc_qoi_panel_eval(mgmc_handle* h, double* out) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (!out) return fail(h, MGMC_E_INVALID, "null argument");
    if (h->qp_K == 0) return fail(h, MGMC_E_INVALID, "no QoI panel installed (mgmc_qoi_panel_set)");
    HIPCHK(h, hipSetDevice(h->device));
    launch_panel(h, nullptr, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->qp_out, (size_t)h->nchains * h->qp_K * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGMC_OK;
}

int mgmc_qoi_panel_record_enable(mgmc_handle* h, int stride, int window, int64_t capacity) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (h->qp_K == 0) return fail(h, MGMC_E_INVALID, "no QoI panel installed (mgmc_qoi_panel_set)");
    if (stride < 1) return fail(h, MGMC_E_INVALID, "QoI panel record: stride must be >= 1");
    if (window < 1 || window > QP_MAX_W) return fail(h, MGMC_E_INVALID, "QoI panel record: window must be in [1, 256]");
    if (capacity < 1) return fail(h, MGMC_E_INVALID, "QoI panel record: capacity must be >= 1");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->qp_ctl && (uint64_t)capacity == h->qp_cap && window == h->qp_window)
        return panel_zero(h, stride);  // a reset (same graphs)
    PanelAllocs al;
    PanelRecordBufs rb;
    if (!panel_record_alloc(h, al, h->qp_K, window, (uint64_t)capacity, &rb))
        return fail(h, MGMC_E_NOMEM, "device allocation failed (QoI panel record)");
    destroy_graphs(h);  // (an enabled handle's hold the old buffers' addresses)
    panel_free_record(h);
    al.keep = true;
    panel_take_record(h, rb, window, (uint64_t)capacity);
    int rc = panel_zero(h, stride);
    if (rc == MGMC_OK) {
        sync_fieldstats_op(h);
        rc = build_graphs(h);
    }
    if (rc != MGMC_OK) {  // back to the cycle without the op
        const std::string err = h->last_error;
        destroy_graphs(h);
        panel_free_record(h);
        sync_fieldstats_op(h);
        (void)build_graphs(h);
        return fail(h, rc, err);
    }
    return MGMC_OK;
}

int mgmc_qoi_panel_record_disable(mgmc_handle* h) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (!h->qp_ctl) return MGMC_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    destroy_graphs(h);  // they hold the buffers' addresses
    panel_free_record(h);
    sync_fieldstats_op(h);
    return build_graphs(h);
}

int mgmc_qoi_panel_record_reset(mgmc_handle* h) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (!h->qp_ctl) return fail(h, MGMC_E_INVALID, "the QoI panel record is not enabled (mgmc_qoi_panel_record_enable)");
    HIPCHK(h, hipSetDevice(h->device));
    return panel_zero(h, h->qp_stride);
}

int mgmc_qoi_panel_info(const mgmc_handle* h, int* K, int* enabled, int* stride, int* window, uint64_t* ncycles,
                        uint64_t* nrecorded) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (K) *K = h->qp_K;
    if (enabled) *enabled = h->qp_ctl ? 1 : 0;
    if (stride) *stride = h->qp_stride;
    if (window) *window = h->qp_window;
    uint64_t cnt[2] = {0, 0};
    if (h->qp_ctl && (ncycles || nrecorded)) {
        int rc = panel_counters(h, cnt);
        if (rc) return rc;
    }
    if (ncycles) *ncycles = cnt[0];
    if (nrecorded) *nrecorded = cnt[1];
    return MGMC_OK;
}

int mgmc_qoi_panel_get_series(mgmc_handle* h, int chain, double* out, size_t n) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (!h->qp_ctl) return fail(h, MGMC_E_INVALID, "the QoI panel record is not enabled (mgmc_qoi_panel_record_enable)");
    if (chain < 0 || chain >= h->nchains) return fail(h, MGMC_E_INVALID, "chain index out of range");
    if (n && !out) return fail(h, MGMC_E_INVALID, "null argument");
    uint64_t cnt[2];
    int rc = panel_counters(h, cnt);
    if (rc) return rc;
    if (n > std::min(cnt[1], h->qp_cap)) return fail(h, MGMC_E_INVALID, "QoI panel series: more records asked for than kept");
    if (n)
        HIPCHK(h, hipMemcpyAsync(out, h->qp_series + (size_t)chain * h->qp_cap * h->qp_K, n * h->qp_K * sizeof(double),
                                 hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MGMC_OK;
}

int mgmc_qoi_panel_moments(mgmc_handle* h, int chain, double* count, double* mean, double* comoment) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (!h->qp_ctl) return fail(h, MGMC_E_INVALID, "the QoI panel record is not enabled (mgmc_qoi_panel_record_enable)");
    if (chain < 0 || chain >= h->nchains) return fail(h, MGMC_E_INVALID, "chain index out of range");
    HIPCHK(h, hipSetDevice(h->device));
    const int K = h->qp_K;
    std::vector<double> m(panel_mom_doubles(K));
    HIPCHK(h, hipMemcpyAsync(m.data(), h->qp_mom + (size_t)chain * m.size(), m.size() * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (count) *count = m[0];
    if (mean) std::copy(m.begin() + 1, m.begin() + 1 + K, mean);
    if (comoment)  // the device keeps the upper triangle: mirrored here
        for (int k = 0; k < K; ++k)
            for (int l = 0; l < K; ++l) comoment[k * K + l] = m[1 + K + (size_t)std::min(k, l) * K + std::max(k, l)];
    return MGMC_OK;
}

int mgmc_qoi_panel_autocov(mgmc_handle* h, int chain, double* S, int* nlags) {
    if (!h) return fail(nullptr, MGMC_E_INVALID, "null handle");
    if (!h->qp_ctl) return fail(h, MGMC_E_INVALID, "the QoI panel record is not enabled (mgmc_qoi_panel_record_enable)");
    if (chain < 0 || chain >= h->nchains) return fail(h, MGMC_E_INVALID, "chain index out of range");
    uint64_t cnt[2];
    int rc = panel_counters(h, cnt);
    if (rc) return rc;
    if (nlags) *nlags = (int)std::min<uint64_t>(cnt[1], (uint64_t)h->qp_window);
    if (S) {
        const size_t n = (size_t)h->qp_K * h->qp_window;
        HIPCHK(h, hipMemcpyAsync(S, h->qp_S + (size_t)chain * n, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return MGMC_OK;
}

}  // extern "C"
