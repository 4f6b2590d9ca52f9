// pt_culling_state.hpp — the state of the visibility system (pt_culling_passes.cpp), shared with the rasteriser over its
// draw lists (pt_raster_passes.cpp).  Private to the library's translation units.
#pragma once

#include <vector>

#include "pt_context.hpp"
#include "pt_culling.hpp"

namespace ppt
{

struct CullingPassState
{
    // HierarchicalDepthDownsampler keeps two storage sets: the G-buffer's pyramid before and after the second culling phase
    struct HizSlot
    {
        DeviceBuffer pyramid;
        DeviceBuffer hostDepth; // the device copy of a caller's host depth
        HizLayout layout = {};
        uint32_t sourceWidth = 0, sourceHeight = 0, launches = 0;
        bool valid = false;
        Fence done; // behind the last call's kernels: a call or a reader on another stream waits for it
    };
    HizSlot hiz[2];
    int32_t keptHiz = -1; // prosper_pt_cull_gbuffer: the slot whose pyramid is the next call's previous one

    // ---- the draw lists of the last culling calls (MeshletCuller's buffers): grow-only ----
    DeviceBuffer lists[PROSPER_PT_DRAW_LIST_COUNT]; // count, then `capacity` pairs
    DeviceBuffer argsAndStats;                      // two argument triples (first, second phase), then DrawListStats
    DeviceBuffer meshletCounts;                     // [meshCount], what the generator reads
    std::vector<uint32_t> hostMeshletCounts;
    bool countsDirty = true;                        // hostMeshletCounts differs from what the device holds
    uint32_t capacity = 0;   // pairs each list has room for
    uint32_t upperBound = 0; // of the last first phase
    bool listValid[PROSPER_PT_DRAW_LIST_COUNT] = {};
    prosper_pt_draw_stats totals = {}; // the host's part of DrawStats, of the last first phase
    Pinned<DrawListStats> statsHost;
    Fence statsDone; // behind the copy into statsHost
    bool statsQueued = false;
    Fence done;      // behind the last call's kernels
    // the meshlet ranges were checked for this geometry generation
    const void *checkedGeometry = nullptr;
    uint32_t checkedInstalls = 0, checkedUpdates = 0;
    bool checked = false;
    // device time of the last phases' kernels: generator, first-phase culler | second-phase culler
    StageEvents<2> firstTiming;
    StageEvents<1> secondTiming;
    bool firstTimed = false, secondTimed = false;
};

} // namespace ppt
