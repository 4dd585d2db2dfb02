// chroma_launch.hpp -- declarations shared by kernels_chroma.hip (device code) and chroma.hip (host C ABI).
#pragma once

#include "chroma_core.hpp"
#include "kernels.hpp"

namespace v1c {

// what a launch of the chromatic-aberration kernels needs besides its units: launch-invariant and plan-resident -- the kernels read the
// plan's device copy through a constant-address-space reference, like the tile kernels read KernelCtx (kernels.hpp: TileArgs)
struct CaCtx {
    Geom g;                   // cn = 3
    const v1c_chain* chains;  // device copy of the three lowered chains, B, G, R (literal / fix-up modes)
    RayParams ray;            // the shared head of the ray path (green's; its main-table fields are green's too)
    CaTable tab[3];           // the main table of B, G, R
    const short* itab;        // cubic / lanczos4 weight table (device), else null
    uint32_t* tile_flags;     // one word per (unit slot, tile): set by MODE_RAY, consumed by MODE_FIXUP
};

// the ONE by-value kernel argument: the plan's context and the launch's units (DevUnit::rot = the EFFECTIVE rotation of the ray path:
// the unit's override or the chain's composed one)
struct CaArgs {
    const CaCtx* ctx;
    DevUnit u[kMaxUnitsPerLaunch];
};

// `mode`: MODE_LITERAL / MODE_RAY / MODE_FIXUP (kernels.hpp); `c`: the host copy of the context (geometry of the grid)
hipError_t launch_remap_ca(int mode, const CaCtx& c, const CaArgs& a, int n_units, hipStream_t stream);
// the float32 map of one channel (0 B, 1 G, 2 R) for unit 0 of `a`; `mode`: MODE_LITERAL / MODE_RAY
hipError_t launch_get_map_ca(int mode, const CaCtx& c, const CaArgs& a, int channel, float* xmap, float* ymap, int64_t pitch,
                             hipStream_t stream);

}  // namespace v1c
