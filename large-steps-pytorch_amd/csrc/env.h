// env.h -- the environment variables the native library reads. env.cpp is the only source of csrc/ that calls getenv
// (csrc/experiments/ aside); tests/test_abi_and_host.py holds the two to each other. Nothing is cached: every call reads the environment
// again, because tests and tuning runs change the variables between two constructions of one process.
#pragma once
#include <optional>

namespace ls {

bool env_debug();                                  // LS_DEBUG set: print a stale HIP error found on entry to the library
bool env_plan_timing();                            // LS_PLAN_TIMING set: the constructors' stage clock on stderr
double env_pool_gb();                              // LS_POOL_GB (unset: 24; <= 0: no pool), read at every hand-back to the pool
// LS_PLAN_THREADS (unset: dflt), at most the host's cores; per_rank: the cores divided among the ranks of one node
// (LOCAL_WORLD_SIZE, else WORLD_SIZE)
int env_plan_threads(int dflt, bool per_rank);

// knobs of one nested-dissection construction: read once at the entry of a constructor and passed down
struct NdEnv {
    int order;                        // LS_ND_ORDER clamped to [-1, 1]; unset: -1 (ND_ORDER_AUTO)
    double suspect;                   // LS_ND_SUSPECT (unset or <= 0: 1.3): the spread above which ND_ORDER_AUTO tries the trial cuts too
    std::optional<int> tier_waves;    // LS_ND_TIER_WAVES (any integer; an explicit ls_direct_options / ls_direct_arrays value wins)
    bool host_embed;                  // LS_ND_HOST_EMBED set: the graph embedding by the host's sweeps instead of the device's
    bool no_small, no_pack;           // LS_ND_NO_SMALL / LS_ND_NO_PACK set: no LDS-staged / no packed level kernels
    int long_red;                     // LS_ND_LONG (unset or <= 0: 64): down-sweep reduction from which lanes run along it
    int long_up;                      // LS_ND_LONG_UP (unset or <= 0: 0, the level count's rule)
    int steps;                        // LS_ND_STEPS (unset or <= 0: 128): reduction steps per wave of the row-per-lane down kernel
};
NdEnv nd_env();

}  // namespace ls
