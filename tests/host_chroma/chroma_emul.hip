// chroma_emul.hip -- the chromatic-aberration plan's host logic (csrc/chroma_plan.hpp) and per-pixel code (csrc/chroma_core.hpp)
// compiled for the HOST: which channel chains fuse, and ray_eval3 against ray_eval over every pixel of an output.
#include <cstring>

#include "../../vr180_convert_amd/csrc/chroma_plan.hpp"

using namespace v1c;

namespace {

RadialTable fit_direct(const TableSpec& sp)
{
    return build_radial_table(*sp.stages, sp.n_int, sp.fn, sp.m_max, sp.force_var, sp.m_front);
}

// the RayParams of a plan of ONE chain, as plan.hip / tests/host_emul fill them (host pointers)
RayParams params_of(const RayPlanHost& H)
{
    const RayAnalysis& a = H.a;
    const RayHostTables& ht = H.ht;
    const RadialTable& T = H.table;
    RayParams P{};
    P.col_s = ht.col_s.data(), P.col_c = ht.col_c.data(), P.col_h = ht.col_h.data();
    P.row_s = ht.row_s.data(), P.row_c = ht.row_c.data(), P.row_h = ht.row_h.data();
    P.radial = T.coef.data();
    P.inv_step = T.inv_step, P.n_int = T.n_int, P.var_is_w = T.var_is_w, P.has_rot = a.has_rot;
    for (int q = 0; q < 9; q++)
        P.rot[q] = a.rot[q];
    P.rx = a.rx, P.ry = a.ry, P.cx = a.cx, P.cy = a.cy;
    P.rx32 = 32.0 * a.rx, P.ry32 = 32.0 * a.ry, P.cx32 = 32.0 * a.cx, P.cy32 = 32.0 * a.cy;
    P.n_int_f = (double)P.n_int;
    P.gen_mode = a.gen_mode;
    if (H.has_pre) {
        P.pre_s = H.pre_s.coef.data(), P.pre_c = H.pre_c.coef.data();
        P.pre_var_is_w = H.pre_s.var_is_w, P.pre_inv_step = H.pre_s.inv_step, P.pre_n_int = H.pre_s.n_int;
    }
    return P;
}

bool same_bits(double a, double b)
{
    return std::memcmp(&a, &b, 8) == 0;
}

}  // namespace

extern "C" {

// out[0] = the three chains fuse (1 / 0); out[1 + c] = the channel whose table channel c reads; out[4] = every chain of its own takes the
// ray path today (analysed and usable)
int ca_emul_fuse(const v1c_chain* chains, int w, int h, long long* out)
{
    const CaPlanHost H = build_ca_plan_host(chains, w, h, fit_direct);
    out[0] = H.fused;
    for (int c = 0; c < 3; c++)
        out[1 + c] = H.table_of[c];
    bool each = true;
    for (int c = 0; c < 3; c++)
        each = each && build_ray_plan_host(chains[c], w, h, fit_direct).usable;
    out[4] = each;
    return 0;
}

// ray_eval3 of the fused plan against ray_eval with each channel's OWN single-chain plan, over every pixel.
// out[0] = pixels; out[1] = pixels valid in all three channels by ray_eval; out[2] = pixels where ray_eval3's verdict differs from that;
// out[3] = valid pixels where some coordinate differs in its bits; out[4] = tables of the fused plan that differ from the channel's own
// plan's (coefficients, step, interval count, variable); out[5] = channels invalid at a pixel where others are valid (summed).
// Returns 1 when the chains do not fuse.
int ca_emul_compare(const v1c_chain* chains, int w, int h, long long* out)
{
    const CaPlanHost H = build_ca_plan_host(chains, w, h, fit_direct);
    for (int q = 0; q < 6; q++)
        out[q] = 0;
    if (!H.fused)
        return 1;
    RayPlanHost own[3];
    RayParams P[3];
    CaTable T[3];
    for (int c = 0; c < 3; c++) {
        own[c] = build_ray_plan_host(chains[c], w, h, fit_direct);
        if (!own[c].usable)
            return 2;
        P[c] = params_of(own[c]);
        const RadialTable& t = H.table[c];
        T[c] = CaTable{t.coef.data(), t.inv_step, t.n_int, t.var_is_w};
        const RadialTable& o = own[c].table;
        const bool same = t.coef.size() == o.coef.size() && std::memcmp(t.coef.data(), o.coef.data(), t.coef.size() * 8) == 0 &&
                          t.inv_step == o.inv_step && t.n_int == o.n_int && t.var_is_w == o.var_is_w;
        out[4] += !same;
    }
    const RayParams head = params_of(H.G);
    const RayHostTables& ht = H.G.ht;
    const RayAnalysis& a = H.a[1];
    double R[9];
    for (int q = 0; q < 9; q++)
        R[q] = a.rot[q];
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) {
            double x1[3], y1[3], x3[3] = {0, 0, 0}, y3[3] = {0, 0, 0};
            bool ok1[3];
            int nok = 0;
            for (int c = 0; c < 3; c++) {
                const RayHostTables& hc = own[c].ht;
                ok1[c] = ray_eval(P[c], a.has_rot, R, hc.row_s[j], hc.row_c[j], hc.row_h[j], hc.col_s[i], hc.col_c[i], hc.col_h[i], x1[c], y1[c]);
                nok += ok1[c];
            }
            const bool all1 = nok == 3;
            const bool all3 = ray_eval3(head, T, a.has_rot, R, ht.row_s[j], ht.row_c[j], ht.row_h[j], ht.col_s[i], ht.col_c[i], ht.col_h[i], x3, y3);
            out[0]++;
            out[1] += all1;
            out[2] += all1 != all3;
            out[5] += (nok > 0 && nok < 3) ? 3 - nok : 0;
            if (all1 && all3) {
                bool same = true;
                for (int c = 0; c < 3; c++)
                    same = same && same_bits(x1[c], x3[c]) && same_bits(y1[c], y3[c]);
                out[3] += !same;
            }
        }
    return 0;
}

}  // extern "C"
