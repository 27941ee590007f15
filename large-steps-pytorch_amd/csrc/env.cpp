// env.cpp -- see env.h. Every getenv of the native library.
#include "env.h"

#include <algorithm>
#include <cstdlib>
#include <thread>

namespace ls {
namespace {

bool is_set(const char* name) { return getenv(name) != nullptr; }
// unset or <= 0: dflt
int positive_or(const char* name, int dflt) { const char* e = getenv(name); const int v = e ? atoi(e) : 0; return v > 0 ? v : dflt; }

}  // namespace

bool env_debug() { return is_set("LS_DEBUG"); }

bool env_plan_timing() { return is_set("LS_PLAN_TIMING"); }

double env_pool_gb() {
    // (a 4M-vertex construction leaves 14 GB of scratch + 2.4 GB of factor: with 16 the fronts were evicted every time)
    const char* e = getenv("LS_POOL_GB");
    return e ? atof(e) : 24.0;
}

int env_plan_threads(int dflt, bool per_rank) {
    const char* e = getenv("LS_PLAN_THREADS");
    const int want = e ? atoi(e) : dflt;
    int hw = (int)std::thread::hardware_concurrency();
    if (per_rank) {
        // one process per GPU (torchrun): the N ranks of a node analyse their matrices at the same moment on the same host cores --
        // every rank takes its share (LOCAL_WORLD_SIZE is set by torch.distributed.run; WORLD_SIZE as a fallback on one node)
        const char* lw = getenv("LOCAL_WORLD_SIZE");
        if (!lw) lw = getenv("WORLD_SIZE");
        const int ranks = lw ? atoi(lw) : 1;
        if (hw > 0 && ranks > 1) hw = std::max(1, hw / ranks);
    }
    return std::max(1, std::min(want, hw > 0 ? hw : 1));
}

NdEnv nd_env() {
    NdEnv n;
    const char* order = getenv("LS_ND_ORDER");
    n.order = order ? std::max(-1, std::min(1, atoi(order))) : -1;
    const char* suspect = getenv("LS_ND_SUSPECT");
    const double s = suspect ? atof(suspect) : 1.3;
    n.suspect = s > 0.0 ? s : 1.3;
    const char* waves = getenv("LS_ND_TIER_WAVES");
    if (waves) n.tier_waves = atoi(waves);
    n.host_embed = is_set("LS_ND_HOST_EMBED");
    n.no_small = is_set("LS_ND_NO_SMALL");
    n.no_pack = is_set("LS_ND_NO_PACK");
    n.long_red = positive_or("LS_ND_LONG", 64);
    n.long_up = positive_or("LS_ND_LONG_UP", 0);
    n.steps = positive_or("LS_ND_STEPS", 128);
    return n;
}

}  // namespace ls
