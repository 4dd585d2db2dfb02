// chroma_plan.hpp -- what a chromatic-aberration plan derives from its three channel chains on the host (chroma.hip; the host tests
// run the same function).  Host only.
#pragma once

#include <cstring>

#include "chroma_core.hpp"
#include "radial_fit.hpp"

namespace v1c {

inline bool ca_ops_equal(const std::vector<v1c_op>& a, const std::vector<v1c_op>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(v1c_op)) == 0);
}

// The fuse rule: two analysed chains may share one ray direction per pixel when they agree in every RayAnalysis field except the
// radial composite behind the rotation.
inline bool ca_analyses_fuse(const RayAnalysis& a, const RayAnalysis& b)
{
    if (!a.ok || !b.ok)
        return false;
    if (a.has_rot != b.has_rot || a.base != b.base || a.gen_mode != b.gen_mode || std::memcmp(a.rot, b.rot, sizeof(a.rot)) != 0)
        return false;
    if (a.norm_cx != b.norm_cx || a.norm_cy != b.norm_cy || a.norm_s != b.norm_s || a.has_rows != b.has_rows || a.row_lo != b.row_lo ||
        a.row_hi != b.row_hi)
        return false;
    if (a.rx != b.rx || a.ry != b.ry || a.cx != b.cx || a.cy != b.cy)
        return false;
    return ca_ops_equal(a.pre, b.pre);
}

struct CaPlanHost {
    bool fused = false;  // all three chains analysed, equal up to `radial`, every table usable
    RayPlanHost G;       // green's plan: row / column tables, the S / Cm tables, steps and reaches shared by the three channels
    RadialTable table[3];  // the main table per channel, B, G, R (copies where a channel's radial composite equals green's)
    int table_of[3] = {0, 1, 2};  // the channel whose table a channel reads: 1 where its composite equals green's
    RayAnalysis a[3];
};

// `fit`: RadialTable(const TableSpec&), as build_ray_plan_host takes it.  Green's plan is built whole; the other channels get the main
// table green's recipe gives for their own radial composite (same function, interval count, range and front).
template <typename Fit>
inline CaPlanHost build_ca_plan_host(const v1c_chain* chains, int dst_w, int dst_h, Fit&& fit)
{
    CaPlanHost H;
    for (int c = 0; c < 3; c++)
        H.a[c] = analyze_chain(chains[c]);
    if (!ca_analyses_fuse(H.a[1], H.a[0]) || !ca_analyses_fuse(H.a[1], H.a[2]))
        return H;
    H.G = build_ray_plan_host(chains[1], dst_w, dst_h, fit);
    if (!H.G.usable)
        return H;
    H.table[1] = H.G.table;
    const bool planar = H.a[1].base == 1 && !H.a[1].has_rot;
    for (int c = 0; c < 3; c += 2) {
        if (ca_ops_equal(H.a[c].radial, H.a[1].radial)) {
            H.table_of[c] = 1;
            H.table[c] = H.G.table;
            continue;
        }
        if (c == 2 && ca_ops_equal(H.a[2].radial, H.a[0].radial) && H.table_of[0] == 0) {
            H.table_of[2] = 0;
            H.table[2] = H.table[0];
            continue;
        }
        // (build_ray_plan_host's two recipes for the main table)
        if (planar) {
            const double m_max = std::max(H.G.ht.m_reach * 1.05, 1e-6);
            H.table[c] = fit(TableSpec{&H.a[c].radial, FN_PLANAR_G, table_intervals_for(H.G.step, m_max), m_max, -1, H.G.ht.m_reach});
            if (!ray_table_usable(H.table[c], H.G.ht.m_reach, 3))
                return H;
        } else {
            H.table[c] = fit(TableSpec{&H.a[c].radial, FN_RAY_G, table_intervals_for(H.G.step), kTableMMax, -1, 0.0});
            if (!ray_table_usable(H.table[c]))
                return H;
        }
    }
    H.fused = true;
    return H;
}

}  // namespace v1c
