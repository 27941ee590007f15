"""
The meshes of tests/test_meshgeom_scale_gpu.py and what they cross in csrc/meshgeom.hip and in k_gather_corners of csrc/meshface.h.

The constants that set the thresholds are READ from the sources the library is compiled from (normals_scale_cases.compiled_int; VG from
the launch `k_voronoi_mass_gather<IDX, 4>`), not restated, and the case lists below are FORMULAS of them. What every case crosses is
asserted by tests/test_meshgeom_scale_cpu.py with the functions of this file (partials, trips, last_trip): a change of BLOCK, MESH_MAXG,
GC or VG -- or of how the kernels use them (USES) -- fails there instead of silently un-testing the second trip / the tail loop.

    sweep   the first F' faces of jittered_plane(514) around one and two sweeps of k_edge_length_partials's capped grid, and the whole
            jittered_plane(364): a face dropped or counted twice at a trip boundary
    small   F' around one wave, one workgroup, two workgroups: one partial, two partials, a last workgroup with one face
    ladder  open fans of 1 .. 13 triangles and one of 4 BLOCK + 7: every remainder of the valence modulo VG and GC (each clamp position
            of the two request groups), valences past GC (the tail loop of k_gather_corners) and one past BLOCK
    pad     V around one workgroup of the per-vertex kernels, and F' = 128 (36 F' a multiple of 512) with three trailing unreferenced
            vertices
A sliced mesh keeps every vertex of its plane: the ones the slice does not use are unreferenced trailing vertices.
"""
import functools
import re

import numpy as np

import normals_scale_cases as nc

BLOCK = nc.BLOCK
WAVE = nc.compiled_int("common.h", "WAVE")
MESH_MAXG = nc.MESH_MAXG
GC = nc.compiled_int("meshface.h", "GC")           # corners k_gather_corners requests together before its tail loop


def launched_vg():
    """VG of k_voronoi_mass_gather as ls_massmatrix_voronoi launches it; exactly one launch, or an error"""
    found = re.findall(r"k_voronoi_mass_gather<\s*IDX\s*,\s*(\d+)\s*>", nc.source("meshgeom.hip"))
    if len(found) != 1:
        raise AssertionError(f"meshgeom.hip: expected one launch `k_voronoi_mass_gather<IDX, <literal>>`, found {len(found)}")
    return int(found[0])


VG = launched_vg()                                  # corners a thread of k_voronoi_mass_gather requests together, group after group
SWEEP = MESH_MAXG * BLOCK                           # faces one sweep of k_edge_length_partials's capped grid covers
# how the sources use them: the statements the formulas of this file stand for
USES = {"meshgeom.hip": ["for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * BLOCK)",
                         "const int G = F > 0 ? reduce_grid(F) : 0;",
                         "for (int g = threadIdx.x; g < G; g += MG_FIN) acc += part[g];",
                         "for (int eb = e0; eb < e1; eb += VG)",
                         "cid[t] = order[min(eb + t, e1 - 1)]",
                         "dim3(div_up(V, BLOCK)), dim3(BLOCK), 0, st, verts, (const IDX*)faces, V"],
        "meshface.h": ["std::min<int64_t>(MESH_MAXG, std::max<int64_t>(1, div_up(F, BLOCK)))",
                       "const size_t e = (size_t)min(e0 + t, last);",
                       "for (int e = e0 + GC; e < e1; ++e)",
                       "dim3(div_up(V, BLOCK)), dim3(BLOCK), 0, st, vptr, corner, V, dst, out"]}

PLANE, PLANE_2 = 514, 364                           # the sliced plane (2 * 513^2 = 526338 faces) and the one taken whole
HUB = 4 * BLOCK + 7                                 # the ladder's large fan
LADDER_FANS = tuple(range(1, 14)) + (HUB,)
PAD_PLANE = 15


def partials(F):
    """G = reduce_grid(F): the workgroups of k_edge_length_partials, one partial sum each"""
    return min(MESH_MAXG, max(1, -(-F // BLOCK)))


def trips(F):
    """the trips thread 0 of workgroup 0 makes through the loop of k_edge_length_partials (no thread makes more)"""
    return -(-F // (partials(F) * BLOCK))


def last_trip(F):
    """the faces of the last trip: F minus what the trips before it cover"""
    return F - (trips(F) - 1) * partials(F) * BLOCK


SWEEP_SIZES = (SWEEP - 1, SWEEP, SWEEP + 1, SWEEP + BLOCK, SWEEP + BLOCK + 1, 2 * SWEEP, 2 * SWEEP + 1, 2 * (PLANE - 1) ** 2)
SMALL_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
PAD_SIZES = (BLOCK - 1, BLOCK, BLOCK + 1)

SWEEP_CASES = tuple(f"sweep{F}" for F in SWEEP_SIZES) + (f"sweep_plane{PLANE_2}",)
SMALL_CASES = tuple(f"small{F}" for F in SMALL_SIZES)
PAD_CASES = tuple(f"pad{V}" for V in PAD_SIZES) + ("pad_f128",)
CASES = SWEEP_CASES + SMALL_CASES + ("ladder",) + PAD_CASES


@functools.lru_cache(maxsize=None)
def _plane(n):
    v, f = nc.jittered_plane(n)
    v.setflags(write=False), f.setflags(write=False)
    return v, f


def ladder(seed=11):
    """open fans of k triangles for k in LADDER_FANS, side by side: the apex of fan k has valence k and sits in slot t % 3 of the fan's
    t-th triangle; the rim (radius 1 around the apex, steps of min(0.4, 5 / k) rad) has a seeded radial jitter of +-0.3 rim steps and a
    little height; then a seeded permutation of the vertices and of the faces. fp32 verts, int64 faces."""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for i, k in enumerate(LADDER_FANS):
        step = min(0.4, 5.0 / k)
        ang = step * np.arange(k + 1)
        r = 1.0 + 0.3 * step * rng.uniform(-1.0, 1.0, k + 1)
        rim = np.stack([r * np.cos(ang), r * np.sin(ang), 0.1 * step * rng.uniform(-1.0, 1.0, k + 1)], 1)
        base = sum(len(x) for x in verts)
        verts.append(np.concatenate([[[0.0, 0.0, 0.25]], rim]) + np.array([3.0 * i, 0.0, 0.0]))
        for t in range(k):
            tri = [base, base + 1 + t, base + 2 + t]
            faces.append(tri[-(t % 3):] + tri[:-(t % 3)] if t % 3 else tri)        # the apex in slot t % 3, the orientation kept
    v, f = np.concatenate(verts), np.array(faces, dtype=np.int64)
    new_id = rng.permutation(v.shape[0])
    out = np.empty_like(v)
    out[new_id] = v
    return out.astype(np.float32), new_id[f][rng.permutation(f.shape[0])]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts (V, 3) fp32, faces (F, 3) int64) of a case, read-only"""
    if name == "ladder":
        v, f = ladder()
    elif name == f"sweep_plane{PLANE_2}":
        v, f = _plane(PLANE_2)
    elif name.startswith("sweep") or name.startswith("small"):
        v, f = _plane(PLANE)
        f = f[:int(name[5:])]
    elif name == "pad_f128":
        v, f = _plane(PAD_PLANE)
        f = f[:128]
        v = v[:f.max() + 1 + 3]
    elif name.startswith("pad"):
        v, f = _plane(PAD_PLANE)
        extra = np.random.default_rng(13).uniform(-1.0, 1.0, (int(name[3:]) - v.shape[0], 3)).astype(np.float32)
        v = np.concatenate([v, extra])
    else:
        raise KeyError(name)
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f)
    v.setflags(write=False), f.setflags(write=False)
    return v, f


def valence(name):
    v, f = mesh(name)
    return np.bincount(f.reshape(-1), minlength=v.shape[0])


def mass_weights(name):
    """the seeded normal output gradient of massmatrix_voronoi, (V,) fp32"""
    return np.random.default_rng(17).standard_normal(mesh(name)[0].shape[0]).astype(np.float32)


AVG_WEIGHTS = (1.0, -2.5)                            # the output gradients of average_edge_length
