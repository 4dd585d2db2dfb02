// chroma.hip -- host side of the chromatic-aberration entry points of the C ABI (v1c_ca_plan_*, include/vr180_remap.h): a plan over
// three channel chains (B, G, R) of one BGR remap.  When the chains fuse (chroma_plan.hpp) the plan owns one set of row / column
// tables and one radial table per distinct radial composite; otherwise three interpreters serve it.  v1c_ca_plan_run only fills
// kernel arguments and launches.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "chroma_launch.hpp"
#include "chroma_plan.hpp"
#include "host_util.hpp"

using namespace v1c;

namespace v1c {
RadialTable cached_radial_table_for(const TableSpec& sp);  // plan.hip: the per-process cache of fits
}

#define CA_HIP_TRY(expr)                                                                                \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return set_error(V1C_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

struct v1c_ca_plan {
    int device = 0;
    int mode = MODE_LITERAL;
    v1c_chain chains[3]{};
    RayAnalysis ana;               // green's (the channels agree in everything the launches read of it)
    RadialTable table[3];
    int n_rot_stages = 0;          // of every chain (they agree, or units may not override the rotation)
    bool rot_stages_agree = true;
    bool ray_no_rot_safe = false;    // as in v1c_plan, for all three tables
    bool ray_plan_rot_safe = false;
    bool front_hemisphere = false;
    CaCtx ctx{};                   // host copy ...
    const CaCtx* ctx_dev = nullptr;  // ... and the plan-resident device copy the kernels read
    int tiles = 0;
    // the tile-flag words between a ray pass and its fix-up pass: per plan, serialised across streams like v1c_plan's
    std::mutex flags_mu;
    hipEvent_t flags_ev = nullptr;
    hipStream_t flags_stream = nullptr;
    bool flags_pending = false;
    std::atomic<int> last_launch{-1};
    std::vector<void*> allocs;
};

namespace {

int validate_chain(const v1c_chain* ch)
{
    if (ch->n_ops < 1 || ch->n_ops > V1C_MAX_OPS)
        return set_error(V1C_E_INVALID, "chain.n_ops out of range");
    for (int i = 0; i < ch->n_ops; i++) {
        const v1c_op& op = ch->ops[i];
        if (op.opcode < V1C_OP_NORMALIZE || op.opcode > V1C_OP_ROTATE)
            return set_error(V1C_E_INVALID, "unknown opcode in chain");
        if (op.nparam < 0 || op.nparam > V1C_MAX_PARAMS)
            return set_error(V1C_E_INVALID, "op.nparam out of range");
        if (op.opcode == V1C_OP_RADIAL && (op.iparam < V1C_RAD_ENC_RECTILINEAR || op.iparam > V1C_RAD_RECTDEC_INV))
            return set_error(V1C_E_INVALID, "unknown radial kind in chain");
    }
    return V1C_OK;
}

int validate_geom(int src_h, int src_w, int dst_h, int dst_w, int interp, int border)
{
    if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0)
        return set_error(V1C_E_INVALID, "image sizes must be positive");
    if (src_h >= 32768 || src_w >= 32768 || dst_h >= 32768 || dst_w >= 32768)
        return set_error(V1C_E_INVALID, "image sizes must be < 32768 (cv2.remap limit)");
    if (interp < V1C_INTER_NEAREST || interp > V1C_INTER_LANCZOS4)
        return set_error(V1C_E_INVALID, "unknown interpolation");
    if (border < V1C_BORDER_CONSTANT || border > V1C_BORDER_TRANSPARENT)
        return set_error(V1C_E_INVALID, "unknown border mode");
    return V1C_OK;
}

template <typename T>
int upload(v1c_ca_plan* p, const T* h, size_t n, const T** out)
{
    void* d = nullptr;
    CA_HIP_TRY(hipMalloc(&d, std::max<size_t>(n * sizeof(T), 16)));
    p->allocs.push_back(d);
    if (n)
        CA_HIP_TRY(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)d;
    return V1C_OK;
}

int tiles_of(const Geom& g)
{
    return ((g.dst_w + kBlockX * kPX - 1) / (kBlockX * kPX)) * ((g.dst_h + kBlockY - 1) / kBlockY);
}

// everything of the fused form: tables up, the shared head and the three table records into the context
int make_fused(v1c_ca_plan* p, const CaPlanHost& H)
{
    const RayAnalysis& a = H.a[1];
    const RayHostTables& ht = H.G.ht;
    RayParams& r = p->ctx.ray;
    int rc;
    {
        std::vector<double> all;
        all.reserve(3 * ht.col_s.size() + 3 * ht.row_s.size());
        for (const std::vector<double>* v : {&ht.col_s, &ht.col_c, &ht.col_h, &ht.row_s, &ht.row_c, &ht.row_h})
            all.insert(all.end(), v->begin(), v->end());
        const double* base = nullptr;
        if ((rc = upload(p, all.data(), all.size(), &base)))
            return rc;
        const size_t wpad = ht.col_s.size(), hh = ht.row_s.size();
        r.col_s = base, r.col_c = base + wpad, r.col_h = base + 2 * wpad;
        r.row_s = base + 3 * wpad, r.row_c = base + 3 * wpad + hh, r.row_h = base + 3 * wpad + 2 * hh;
    }
    // one upload per distinct radial composite; a channel equal to another reads that one's
    for (int c = 0; c < 3; c++) {
        p->table[c] = H.table[c];
        if (H.table_of[c] != c)
            continue;
        CaTable& t = p->ctx.tab[c];
        if ((rc = upload(p, H.table[c].coef.data(), H.table[c].coef.size(), &t.radial)))
            return rc;
        t.inv_step = H.table[c].inv_step, t.n_int = H.table[c].n_int, t.var_is_w = H.table[c].var_is_w;
    }
    for (int c = 0; c < 3; c++)
        if (H.table_of[c] != c)
            p->ctx.tab[c] = p->ctx.tab[H.table_of[c]];
    r.gen_mode = a.gen_mode;
    if (H.G.has_pre) {
        if ((rc = upload(p, H.G.pre_s.coef.data(), H.G.pre_s.coef.size(), &r.pre_s)) ||
            (rc = upload(p, H.G.pre_c.coef.data(), H.G.pre_c.coef.size(), &r.pre_c)))
            return rc;
        r.pre_var_is_w = H.G.pre_s.var_is_w, r.pre_inv_step = H.G.pre_s.inv_step, r.pre_n_int = H.G.pre_s.n_int;
    }
    r.radial = p->ctx.tab[1].radial, r.inv_step = p->ctx.tab[1].inv_step, r.n_int = p->ctx.tab[1].n_int, r.var_is_w = p->ctx.tab[1].var_is_w;
    r.n_int_f = (double)r.n_int;
    r.has_rot = a.has_rot;
    for (int q = 0; q < 9; q++)
        r.rot[q] = a.rot[q];
    r.rx = a.rx, r.ry = a.ry, r.cx = a.cx, r.cy = a.cy;
    r.rx32 = 32.0 * a.rx, r.ry32 = 32.0 * a.ry, r.cx32 = 32.0 * a.cx, r.cy32 = 32.0 * a.cy;
    r.radial_m = nullptr, r.mp_first_ok = r.n_int, r.inv_step_f = (float)r.inv_step;
    p->front_hemisphere = ht.front_hemisphere;
    p->ray_no_rot_safe = !a.has_rot;
    p->ray_plan_rot_safe = a.has_rot && H.G.reach_rot < 2.0 && H.G.pre_safe;
    for (int c = 0; c < 3; c++) {
        p->ray_no_rot_safe = p->ray_no_rot_safe && ray_reach_is_safe(p->table[c], H.G.reach_norot);
        p->ray_plan_rot_safe = p->ray_plan_rot_safe && ray_reach_is_safe(p->table[c], H.G.reach_rot);
    }
    // tile flags for kMaxUnitsPerLaunch units
    const size_t nflag = (size_t)p->tiles * kMaxUnitsPerLaunch;
    const std::vector<uint32_t> zeros(nflag, 0u);
    const uint32_t* flags = nullptr;
    if ((rc = upload(p, zeros.data(), nflag, &flags)))
        return rc;
    p->ctx.tile_flags = (uint32_t*)flags;
    CA_HIP_TRY(hipEventCreateWithFlags(&p->flags_ev, hipEventDisableTiming));
    p->mode = MODE_RAY;
    return V1C_OK;
}

int fill_unit(const v1c_ca_plan* p, const v1c_unit& in, DevUnit& out)
{
    if (!in.src || !in.dst)
        return set_error(V1C_E_INVALID, "unit src/dst is NULL");
    const Geom& g = p->ctx.g;
    if (in.src_pitch < (int64_t)g.src_w * 3 || in.dst_pitch < (int64_t)g.dst_w * 3)
        return set_error(V1C_E_INVALID, "unit pitch smaller than a row");
    if (in.has_rot && (p->n_rot_stages == 0 || !p->rot_stages_agree))
        return set_error(V1C_E_INVALID, "unit carries a rotation but the plan's chains have no rotate stage (or not the same number of them)");
    out.src = in.src, out.dst = in.dst;
    out.src_pitch = in.src_pitch, out.dst_pitch = in.dst_pitch;
    out.has_rot = in.has_rot ? 1 : 0;
    out.pad = 0;
    const bool plan_rot = p->mode == MODE_RAY && p->ana.has_rot;
    for (int q = 0; q < 9; q++)
        out.rot[q] = in.has_rot ? in.rot[q] : (plan_rot ? p->ana.rot[q] : 0.0);
    return V1C_OK;
}

// the by-value argument block of the kernels: the plan-resident context and up to kMaxUnitsPerLaunch records
CaArgs unit_args(const v1c_ca_plan* p, const DevUnit* du, int n)
{
    CaArgs ua;
    std::memset(&ua, 0, sizeof(ua));
    ua.ctx = p->ctx_dev;
    std::memcpy(ua.u, du, sizeof(DevUnit) * (size_t)n);
    return ua;
}

// units that override the rotation: the interpreter where the plan's proofs hold for its own rotation only (v1c_plan_run's rule)
bool units_take_literal(const v1c_ca_plan* p, bool any_rot)
{
    return p->mode != MODE_RAY || (any_rot && (p->n_rot_stages > 1 || p->ana.gen_mode != 0));
}

// whether a fix-up pass must follow the ray pass over these units (decide_launch of plan.hip, for three tables)
bool need_fixup(const v1c_ca_plan* p, const DevUnit* du, int n, bool any_rot)
{
    if (!any_rot)
        return !(p->ray_no_rot_safe || p->ray_plan_rot_safe);
    if (!p->front_hemisphere)
        return true;
    for (int k = 0; k < n; k++) {
        const double* r = du[k].has_rot ? du[k].rot : p->ana.rot;
        const bool rotated = du[k].has_rot || p->ana.has_rot;
        if (!rotated) {
            if (!p->ray_no_rot_safe)
                return true;
            continue;
        }
        for (int c = 0; c < 3; c++)
            if (!ray_reach_is_safe(p->table[c], rotated_reach(r)))
                return true;
    }
    return false;
}

}  // namespace

extern "C" int v1c_ca_plan_destroy(v1c_ca_plan* p)
{
    if (!p)
        return V1C_OK;
    DeviceGuard dg(p->device);
    for (void* d : p->allocs)
        (void)hipFree(d);
    if (p->flags_ev)
        (void)hipEventDestroy(p->flags_ev);
    delete p;
    return V1C_OK;
}

extern "C" int v1c_ca_plan_create(v1c_ca_plan** out, int device, const v1c_chain chains[3], int src_h, int src_w, int dst_h, int dst_w,
                                  int interp, int border_mode, const uint8_t border_val[4])
{
    if (!out)
        return set_error(V1C_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!chains)
        return set_error(V1C_E_INVALID, "chains is NULL");
    int rc;
    for (int c = 0; c < 3; c++)
        if ((rc = validate_chain(&chains[c])))
            return rc;
    if ((rc = validate_geom(src_h, src_w, dst_h, dst_w, interp, border_mode)))
        return rc;
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");

    v1c_ca_plan* p = new v1c_ca_plan();
    p->device = device;
    Geom& g = p->ctx.g;
    g.src_h = src_h, g.src_w = src_w, g.dst_h = dst_h, g.dst_w = dst_w;
    g.cn = 3;
    g.interp = interp == V1C_INTER_AREA ? V1C_INTER_LINEAR : interp;  // cv2.remap: AREA -> LINEAR
    g.border = border_mode;
    for (int k = 0; k < 4; k++)
        g.cval[k] = border_val ? border_val[k] : 0;
    p->tiles = tiles_of(g);
    for (int c = 0; c < 3; c++) {
        p->chains[c] = chains[c];
        int nr = 0;
        for (int i = 0; i < chains[c].n_ops; i++)
            nr += chains[c].ops[i].opcode == V1C_OP_ROTATE;
        if (c == 0)
            p->n_rot_stages = nr;
        else if (nr != p->n_rot_stages)
            p->rot_stages_agree = false;
    }
    auto bail = [&](int code) {
        v1c_ca_plan_destroy(p);
        return code;
    };
    if (g.interp == V1C_INTER_CUBIC || g.interp == V1C_INTER_LANCZOS4) {
        const int K = g.interp == V1C_INTER_CUBIC ? 4 : 8;
        std::vector<int16_t> tab((size_t)1024 * K * K);
        if ((rc = v1c_build_itab(g.interp, tab.data())))
            return bail(rc);
        if ((rc = upload(p, (const short*)tab.data(), tab.size(), &p->ctx.itab)))
            return bail(rc);
    }
    if ((rc = upload(p, p->chains, (size_t)3, &p->ctx.chains)))
        return bail(rc);
    const CaPlanHost H = build_ca_plan_host(p->chains, dst_w, dst_h, [](const TableSpec& sp) { return cached_radial_table_for(sp); });
    p->ana = H.a[1];
    if (H.fused && (rc = make_fused(p, H)))
        return bail(rc);
    if ((rc = upload(p, &p->ctx, (size_t)1, &p->ctx_dev)))  // (complete from here on)
        return bail(rc);
    *out = p;
    return V1C_OK;
}

extern "C" int v1c_ca_plan_path(const v1c_ca_plan* p)
{
    if (!p)
        return set_error(V1C_E_INVALID, "plan is NULL");
    return p->mode == MODE_RAY ? 1 : 0;
}

extern "C" int v1c_ca_plan_last_launch(const v1c_ca_plan* p)
{
    if (!p)
        return set_error(V1C_E_INVALID, "plan is NULL");
    return p->last_launch.load(std::memory_order_relaxed);
}

extern "C" int v1c_ca_plan_run(v1c_ca_plan* p, void* stream, const v1c_unit* units, int n_units)
{
    if (!p || !units || n_units <= 0)
        return set_error(V1C_E_INVALID, "v1c_ca_plan_run: bad arguments");
    std::vector<DevUnit> du((size_t)n_units);
    for (int k = 0; k < n_units; k++) {
        int rc = fill_unit(p, units[k], du[(size_t)k]);
        if (rc)
            return rc;
    }
    DeviceGuard dg(p->device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    for (int base = 0; base < n_units;) {
        const int n = std::min(kMaxUnitsPerLaunch, n_units - base);
        const DevUnit* u = du.data() + base;
        base += n;
        bool any_rot = false;
        for (int k = 0; k < n; k++)
            any_rot |= u[k].has_rot != 0;
        const CaArgs ua = unit_args(p, u, n);
        if (units_take_literal(p, any_rot)) {
            CA_HIP_TRY(launch_remap_ca(MODE_LITERAL, p->ctx, ua, n, st));
            p->last_launch.store(V1C_LAUNCH_CHROMA, std::memory_order_relaxed);
            continue;
        }
        if (!need_fixup(p, u, n, any_rot)) {
            CA_HIP_TRY(launch_remap_ca(MODE_RAY, p->ctx, ua, n, st));
            p->last_launch.store(V1C_LAUNCH_CHROMA, std::memory_order_relaxed);
            continue;
        }
        // ray pass, flag words, fix-up pass: one sequence at a time per plan, in stream order across streams (v1c_plan_run's scheme; a
        // recorded launch neither waits for nor records the plan's event)
        std::lock_guard<std::mutex> flags_lk(p->flags_mu);
        const bool capturing = stream_is_capturing(st);
        if (!capturing && p->flags_pending && p->flags_stream != st)
            CA_HIP_TRY(hipStreamWaitEvent(st, p->flags_ev, 0));
        CA_HIP_TRY(launch_remap_ca(MODE_RAY, p->ctx, ua, n, st));
        CA_HIP_TRY(launch_remap_ca(MODE_FIXUP, p->ctx, ua, n, st));
        if (!capturing) {
            CA_HIP_TRY(hipEventRecord(p->flags_ev, st));
            p->flags_stream = st, p->flags_pending = true;
        }
        p->last_launch.store(V1C_LAUNCH_CHROMA | V1C_LAUNCH_FIXUP, std::memory_order_relaxed);
    }
    return V1C_OK;
}

extern "C" int v1c_ca_plan_get_map(v1c_ca_plan* p, void* stream, int channel, float* xmap, float* ymap, int64_t map_pitch, const double* rot)
{
    if (!p || !xmap || !ymap)
        return set_error(V1C_E_INVALID, "v1c_ca_plan_get_map: bad arguments");
    if (channel < 0 || channel > 2)
        return set_error(V1C_E_INVALID, "channel must be 0 (B), 1 (G) or 2 (R)");
    if (map_pitch < (int64_t)p->ctx.g.dst_w * 4 || (map_pitch & 3))
        return set_error(V1C_E_INVALID, "map_pitch too small or not a multiple of 4");
    if (rot && (p->n_rot_stages == 0 || !p->rot_stages_agree))
        return set_error(V1C_E_INVALID, "rotation given but the plan's chains have no rotate stage");
    DeviceGuard dg(p->device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    DevUnit du;
    std::memset(&du, 0, sizeof(du));
    du.has_rot = rot ? 1 : 0;
    const bool plan_rot = p->mode == MODE_RAY && p->ana.has_rot;
    for (int q = 0; q < 9; q++)
        du.rot[q] = rot ? rot[q] : (plan_rot ? p->ana.rot[q] : 0.0);
    const CaArgs ua = unit_args(p, &du, 1);
    const int mode = units_take_literal(p, rot != nullptr) ? MODE_LITERAL : MODE_RAY;
    CA_HIP_TRY(launch_get_map_ca(mode, p->ctx, ua, channel, xmap, ymap, map_pitch, (hipStream_t)stream));
    return V1C_OK;
}
