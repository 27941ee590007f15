/*
 * largesteps_hip.h -- C ABI of liblargesteps_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of the `largesteps` parameterization hot path. Every entry point takes plain
 * device pointers, sizes, a HIP device ordinal and a hipStream_t passed as void*; no torch types, no
 * C++ types, nothing is thrown across the boundary. Every function returns an int status:
 *       0            success
 *      <0            LS_E_* (invalid argument / state, see below)
 *      >0            a hipError_t raised by the runtime
 * ls_last_error() returns a thread-local human readable message for the last non-zero status.
 *
 * All pointers are DEVICE pointers unless the parameter name starts with `h_` (host).
 * Work is enqueued on `stream`; functions that have to return a size to the host (marked SYNC)
 * synchronise that stream once.
 *
 * Reference interface each entry point replaces (paths relative to rgl-epfl/large-steps-pytorch):
 *   ls_assemble_*        largesteps/geometry.py:65-94  (laplacian_uniform), :3-63 (laplacian_cot),
 *                        :96-133 (compute_matrix: M = a I + b L, coalesced)
 *   ls_csr_from_coo      the implicit COO->CSR conversion inside torch's sparse mm
 *                        (largesteps/parameterize.py:30) for a matrix that was not built by ls_assemble_*
 *   ls_spmv              largesteps/parameterize.py:30  (to_differential: u = M @ v)
 *   ls_solver_*          largesteps/solvers.py:26-39 (CholeskySolver.__init__/solve -> cholespy) and
 *                        :41-126 (ConjugateGradientSolver); one handle == one cached solver object of
 *                        largesteps/parameterize.py:48-59
 *   ls_solver_phase/...  no reference counterpart: the reference is single process / single GPU
 *   ls_direct_*          largesteps/solvers.py:36-39 (CholeskySolver.solve: the two triangular solves of the cholespy /
 *                        CHOLMOD factorisation built at :34) -- re-solve phase of the nested-dissection direct solver
 *   ls_adam_uniform_step largesteps/optimize.py:18-41
 *   ls_face_normals* / ls_vertex_normals*   scripts/geometry.py:91-110 (compute_face_normals), :115-147
 *                        (compute_vertex_normals) and the autograd graph torch records through them -- the consumer
 *                        right after from_differential in every optimisation step (scripts/main.py:178-179)
 *   ls_average_edge_length*   scripts/geometry.py:13-33 (average_edge_length: the remesher's target edge length,
 *                        scripts/main.py:146) and its autograd gradient
 *   ls_massmatrix_voronoi*    scripts/geometry.py:35-89 (massmatrix_voronoi: Voronoi area per vertex, obtuse-triangle rule)
 *                        and its autograd gradient
 *   ls_texture_*         nvdiffrast.torch.texture as scripts/render.py calls it (the backgrounds), with gradients to tex and uv
 *   ls_mip_*             the mipmap filter modes of nvdiffrast.torch.texture and the pixel differentials that choose their level
 *   ls_cube_*            the cube-map mode of nvdiffrast.torch.texture (boundary_mode='cube'), with gradients to tex and the direction
 *   ls_mesh_distance_*   igl.point_mesh_squared_distance / igl.hausdorff (figures/comparison/generate_data.py: the error column)
 *   ls_mesh_ray_*        igl.ray_mesh_intersect, and what igl.ambient_occlusion is built from: rays against the mesh of a distance handle
 *   ls_mesh_winding_*    igl.winding_number / igl.fast_winding_number, the sign of igl.signed_distance: over the same handle
 *   ls_mesh_selfx_*      igl.fast_find_self_intersections: which faces of the handle's mesh cut through each other
 *   ls_iso_*             igl.marching_tets on the Kuhn split of a regular grid: a level set as a mesh, with the gradient to the field
 *   ls_subdiv_*          igl.upsample / igl.loop: midpoint and Loop subdivision as a topology built once and a linear map with its transpose
 *   ls_topo_*            igl.vertex_components / facet_components / boundary_loop / remove_unreferenced: components, loops, component filters
 */
#ifndef LARGESTEPS_HIP_H
#define LARGESTEPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LS_VERSION 110 /* 0.1.1: ls_direct_factor_ex / ls_direct_options (round 6), ls_direct_arrays.tier_waves */

#define LS_OK 0
#define LS_E_INVALID (-1)      /* bad argument (null pointer, negative size, unsupported k, ...) */
#define LS_E_INDEX (-2)        /* a face index is outside [0, V) */
#define LS_E_WORKSPACE (-3)    /* workspace too small */
#define LS_E_OVERFLOW (-4)     /* problem does not fit the int32 index space of the kernels */
#define LS_E_STATE (-5)        /* call sequence violated (e.g. fill before pattern) */
#define LS_E_NOT_CONVERGED (-6) /* solver hit max_iter or a non-finite residual; x holds the last iterate */

#define LS_LAPLACIAN_UNIFORM 0
#define LS_LAPLACIAN_COT 1

int ls_version(void);
const char* ls_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Assembly of M = a*I + b*L as CSR (int32 rowptr/col, fp32 val) + the row-major sorted, duplicate
 * free COO index list torch's coalesce() would produce (geometry.py:133).
 *
 *   1. ls_assemble_workspace_bytes -> size the caller must allocate (device memory)
 *   2. ls_assemble_pattern  (SYNC)  -> fills rowptr[V+1], returns nnz through h_nnz
 *   3. caller allocates col[nnz], val[nnz], coo_idx[2*nnz] (int64: row indices then column indices)
 *   4. ls_assemble_fill             -> writes them (same V, F, workspace); optionally dinv[V] = 1/M_ii
 *
 * faces: (F,3) row-major, index width idx_bytes in {4, 8}. verts: (V,3) fp32 row-major, only read
 * for LS_LAPLACIAN_COT (may be NULL otherwise). `a` and `b` are the already fp32-rounded scalars
 * (a=1,b=lambda  or  a=1-alpha,b=alpha).
 * --------------------------------------------------------------------------------------------- */
int ls_assemble_workspace_bytes(int64_t V, int64_t F, size_t* h_bytes);
int ls_assemble_pattern(const void* faces, int idx_bytes, int64_t F, int64_t V, const float* verts,
                        int kind, float a, float b, void* workspace, size_t workspace_bytes,
                        int32_t* rowptr, int64_t* h_nnz, int device, void* stream);
int ls_assemble_fill(const void* workspace, size_t workspace_bytes, int64_t V, int64_t F, const int32_t* rowptr,
                     int32_t* col, float* val, int64_t* coo_idx, int64_t nnz, float* dinv, int device,
                     void* stream);

/* Foreign matrix: coalesced (row-major sorted, unique) COO int64 -> CSR int32. rowptr[V+1], col[nnz];
 * val is shared with the COO tensor (same order) so only indices are produced. dinv[V] = 1/M_ii optional.
 * scratch: >= 4*(V+1) + 4*((V+1)/2048+4) + 1024 bytes. SYNC (validates sortedness / index range). */
int ls_csr_from_coo(const int64_t* coo_rows, const int64_t* coo_cols, const float* vals, int64_t nnz,
                    int64_t V, int32_t* rowptr, int32_t* col, float* dinv, void* scratch,
                    size_t scratch_bytes, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * y[V,k] = M x[V,k]   (row-major, leading dimension = k, fp32). 1 <= k <= 64.
 * variant: 0 = default (LDS-staged CSR), 1 = thread-per-row direct CSR (kept for A/B measurements).
 * --------------------------------------------------------------------------------------------- */
int ls_spmv(const int32_t* rowptr, const int32_t* col, const float* val, int64_t V, int64_t nnz,
            const float* x, float* y, int k, int variant, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Jacobi-preconditioned conjugate gradient on M (SPD). One handle per matrix; owns a SELL-64 copy of the
 * matrix and its workspace (dinv, r, p, Ap, reduction scratch) sized for `kmax` right-hand-side columns
 * (1..4). The CSR arrays are only read during creation. SYNC (once, to size the SELL copy).
 * --------------------------------------------------------------------------------------------- */
typedef struct ls_solver ls_solver;

typedef struct ls_solve_info {
    int32_t iterations;   /* iterations executed until every column met its threshold (-1: still running, ls_solver_poll) */
    int32_t converged;    /* 1 if every column met its threshold */
    double  rnorm[4];     /* final ||r||_2 per column (recursively updated residual) */
    double  bnorm[4];     /* ||b||_2 per column */
} ls_solve_info;

int ls_solver_create(const int32_t* rowptr, const int32_t* col, const float* val, int64_t V,
                     int64_t nnz, int kmax, int device, void* stream, ls_solver** h_out);
int ls_solver_destroy(ls_solver* s);
/* x0 may be NULL (cold start, x0 = 0). b, x, x0: (V,k) fp32 row-major contiguous; x may alias x0 but not b.
 * A column is converged when ||r||_2 <= max(rtol*||b||_2, atol). SYNC (the host polls convergence).
 * Returns LS_E_NOT_CONVERGED (info still filled) if max_iter is hit. */
int ls_solver_solve(ls_solver* s, const float* b, const float* x0, float* x, int k, double rtol,
                    double atol, int max_iter, ls_solve_info* h_info, void* stream);
/* Chebyshev-accelerated Jacobi iteration on the same handle: one kernel per iteration, no dot products. Needs
 * ls_solver_set_spectrum(s, a_min) with a_min <= lambda_min(M) (M = a I + b L with L positive semi-definite: a);
 * the upper end of spec(D^-1 M) is the handle's own Gershgorin bound. The iteration count is fixed a priori:
 * ceil(log(2/t) / log((sqrt(kappa)+1)/(sqrt(kappa)-1))) for the requested residual reduction t (rtol, or
 * max(rtol||b||, atol)/||r0|| after one residual evaluation when x0 or atol is given). h_info->rnorm is the TRUE
 * fp32 residual of the returned x. SYNC once at the end. LS_E_STATE without a spectrum or with an empty one (a_min /
 * max diag above the Gershgorin bound: no lower bound of the spectrum), LS_E_NOT_CONVERGED if the
 * count exceeds max_iter or the final check fails: ||b - M x|| must be <= max(request, 8 eps32 ||M|| ||x||), the
 * backward-stable fp32 level (callers fall back to ls_solver_solve). */
int ls_solver_set_spectrum(ls_solver* s, double a_min);
/* Declare M = a I + b L_uniform (every off-diagonal entry equals -b): the Chebyshev solver then reads only the
 * neighbour ids (4 B per entry instead of 8 B) -- values are implicit. SYNC once (sizes the column-only SELL copy). */
int ls_solver_set_uniform(ls_solver* s, float a, float b, void* stream);
int ls_solver_spectrum(const ls_solver* s, double* h_lmin, double* h_lmax);
/* Patch plan of the LDS-resident s-step Chebyshev kernel (host arrays, built by largesteps/patches.py; needs
 * ls_solver_set_uniform first): the vertices are renumbered patch-major (h_perm[new] = old); patch p owns the new ids
 * [table[20p], table[20p] + table[20p+1]); one workgroup keeps both iterates of the patch and of its ghost layers 1..depth
 * in LDS and advances `depth` Chebyshev steps per launch, so HBM sees vectors and matrix once per `depth` iterations.
 * table: 20 int32 per patch {own_start, n_own, n_rows, n_local, ell_width, off_gid, off_cols, off_diag, lim[0..11]}
 * (depth <= 12) with
 * lim[m] = number of rows in layers <= m (lim[0] = n_own, lim[m >= depth-1] = n_rows): step j of an S-step launch only
 * recomputes rows < lim[S-1-j], the outer layers are stale by then and never reach an own vertex; h_ghost_gid:
 * new global ids of the local vertices >= n_own; h_cols16: per patch (ell_width, n_rows) uint16 local neighbour ids
 * (padding = n_local); h_diag: per patch the n_rows diagonal entries. SYNC (copies the arrays). */
int ls_solver_set_patches(ls_solver* s, const int32_t* h_table, int n_patches, const int32_t* h_ghost_gid, int64_t n_gid,
                          const uint16_t* h_cols16, int64_t n_cols, const float* h_diag, int64_t n_diag,
                          const int32_t* h_perm, int depth, int max_local, int max_rows, void* stream);
/* iterations the Chebyshev solver will run for a residual reduction `reduction` (e.g. rtol from a cold start) */
int ls_solver_chebyshev_iterations(const ls_solver* s, double reduction, int* h_n);
int ls_solver_solve_chebyshev(ls_solver* s, const float* b, const float* x0, float* x, int k, double rtol,
                              double atol, int max_iter, ls_solve_info* h_info, void* stream);
/* knobs for measurements: name in {"check_every", "grid" (workgroups per kernel, 0 = auto), "block" (0 = auto,
 * 256, 512 or 1024 threads per workgroup), "graph" (1 = replay the Chebyshev launches of a solve as one hipGraph,
 * default; 0 = eager launches), "patch" (1 = use the patch plan if one was set, default), "profile"}; unknown name -> LS_E_INVALID */
int ls_solver_set(ls_solver* s, const char* name, int value);
/* With "profile"=1 every solve brackets its three kernels per iteration with HIP events on the solve's
 * stream; this returns the accumulated milliseconds of K1 (SpMV+dot), K2 (update), K3 (direction) over the h_iters
 * iterations that really ran in the last PCG solve; after a Chebyshev solve: [0] = total of the h_iters launches. */
int ls_solver_profile(const ls_solver* s, double* h_ms3, int* h_iters);
/* the handle's SELL-64 copy of the matrix: slice_ptr[V/64+1] (entry offsets), cv[entries] = {col, fp32 bits} */
int ls_solver_sell(ls_solver* s, const int32_t** h_slice_ptr, const void** h_cv, int64_t* h_entries);
/* bytes the handle allocated on the device */
int ls_solver_workspace_bytes(const ls_solver* s, size_t* h_bytes);

/* ------------------------------------------------------------------------------------------------
 * Vertex-block shard of the same solver (one process per GPU, largesteps/distributed.py). The shard owns
 * rows [0, n_rows) of its block; columns are local ids: [0, n_rows) owned, [n_rows, n_cols) halo. The host
 * driver launches one kernel at a time and, between them, exchanges the halo rows of p and sums the
 * reduction partials across ranks (RCCL):
 *   phase 0  r = b, p = D^-1 r, x = 0 ; partials r.z, r.r, b.b      -> all-reduce partials [1..3]
 *   phase 1  thresholds / column mask from the summed partials
 *   phase 2  K1: Ap = M p_ext ; partial p.Ap  (needs the halo of p)   -> all-reduce partials [0]
 *   phase 3  K2: x += a p ; r -= a Ap ; partials r.z, r.r             -> all-reduce partials [1..2]
 *   phase 4  K3: p = D^-1 r + b p ; publishes the stop flag            -> halo exchange of p
 * ls_solver_buffers exposes p ((n_cols,k) fp32; the halo rows start at p + n_rows*k) and the partial array
 * (4 slots x 4 columns x h_part_stride doubles; slot s, column c, workgroup g at ((s*4+c)*stride + g)); every
 * rank must use the same "grid" so that the partial arrays line up.
 * --------------------------------------------------------------------------------------------- */
int ls_solver_create_ext(const int32_t* rowptr, const int32_t* col, const float* val, int64_t n_rows,
                         int64_t n_cols, int64_t nnz, int kmax, int device, void* stream, ls_solver** h_out);
int ls_solver_phase(ls_solver* s, int phase, const float* b, float* x, int k, double rtol, double atol,
                    int it, void* stream);
int ls_solver_buffers(ls_solver* s, float** h_p, double** h_part, int* h_grid, int* h_part_stride);
/* Replace the handle's p ((n_cols*kmax) floats) and partial array (4*4*stride doubles, zero-initialised by the
 * caller) by caller-owned device buffers, so that the host driver can hand them to its communication library. */
int ls_solver_bind(ls_solver* s, float* p_ext, double* part);
/* Sharded Chebyshev (largesteps/distributed.py ShardedChebyshev): `nsteps` iterations it0..it0+nsteps-1 on the first
 * n_rows rows of the shard (owned rows + redundantly computed ghost layers). xa / xb: (n_cols,k) ping-pong buffers,
 * iteration `it` gathers from (it even ? xa : xb) and overwrites the other; h_c1/h_c2: HOST arrays of the nsteps
 * Chebyshev coefficients (it = 0: x1 = x0 + c2 D^-1 (b - M x0)). No collective is needed between these launches. */
int ls_shard_cheb_steps(ls_solver* s, const float* b, float* xa, float* xb, int k, int it0, int nsteps,
                        const float* h_c1, const float* h_c2, int64_t n_rows, void* stream);
/* partials of ||b - M x||^2 (slots 1 and 2) and ||b||^2 (slot 3) over the first n_rows rows -> all-reduce ->
 * ls_solver_phase(1) -> ls_solver_poll gives the global norms */
int ls_shard_resnorm(ls_solver* s, const float* b, const float* x, int k, int64_t n_rows, void* stream);
/* SYNC: copies the device scalars; h_info->iterations = -1 while no stop was published. */
int ls_solver_poll(ls_solver* s, int k, int n_enqueued, ls_solve_info* h_info, void* stream);
/* dst[t,:] = src[idx[t],:] for t < n (halo send buffer packing), k in 1..4 */
int ls_gather_rows(const float* src, const int32_t* idx, int64_t n, int k, float* dst, int device, void* stream);

/* ---- factor-once / re-solve direct solver (nested dissection, multifrontal; symbolic analysis: csrc/nd_plan.cpp,
 *      numeric factorisation: csrc/nd_factor.hip, re-solve: csrc/direct.hip + csrc/nd_tier.h) ---------
 * The elimination tree is a complete `arity`-ary tree (2, 4 or 8) of `levels` levels; node ids are 1-based and
 * level-major (level l: arity^l nodes, node (l, q) has the children (l+1, arity*q + c)). The vertices are renumbered
 * deepest level first (h_perm[new] = old); node i owns the new ids [own_start, own_start + s) and has b boundary
 * vertices in its ancestors; its front is [own | boundary] and front_off is its offset in the concatenation of all
 * fronts (n_front positions). h_ppos[bnd_off + i] = position of boundary vertex i in the PARENT's front (n_bnd entries).
 * h_push_ptr (n_front + 1) / h_push_tgt (n_bnd): CSR lists, front position -> indices (into the concatenated boundary
 * vectors) of the children's boundary entries that are this vertex.
 * Factor arrays (DEVICE, fp32, owned by the caller and kept alive for the handle's lifetime; the kernels read rows with 16-byte
 * loads that are only 4-byte aligned, so d_finv / d_wf / d_wb need at least 12 readable bytes of slack behind their last entry):
 * d_finv[finv_off + t*s + j] = (F_ss^-1)[t][j]; W = F_bs F_ss^-1 twice: d_wf[w_off + j*b + i] = d_wb[w_off + i*s + j] = W[i][j].
 * h_nodes: (n_nodes + 1, 8) int64, row i = {s, b, own_start, bnd_off, front_off, finv_off, w_off, parent} (row 0 unused).
 * One solve = one launch per upper level upwards
 *     b'_s = b_s - (children's updates at own_i);   upd_i = W_i b'_s + (children's updates at bnd_i)
 * (children push into one slot per child of every parent front position), one launch per upper level downwards
 *     x_s = F_ss^-1 b'_s - W_i^T x[bnd_i]          (parents push x into the children's boundary vectors);
 * the levels stored in the tier layouts run as ONE launch per sweep, a workgroup per subtree (csrc/nd_tier.h).
 * b is read and x written in the caller's numbering. No atomics: bitwise reproducible. A handle owns one workspace:
 * solves issued on different streams are serialised on the device (event wait), concurrent host threads must not
 * share a handle. ls_direct_create is SYNC (copies the host tables). */
/* ---- host-side analysis for the LDS-resident s-step Chebyshev kernel (ls_solver_set_patches; csrc/patch_plan.cpp, host threads, no
 * device): the mesh cut into 2^m equally sized compact patches (recursive coordinate bisection of h_positions, (V, 3)), every patch with
 * its ghost layers 1..depth and patch-local uint16 neighbour ids. h_rowptr / h_col: CSR pattern of M (diagonal included), h_diag: its
 * diagonal. The deepest plan <= depth whose patches keep <= cap_local local vertices (LDS) and <= cap_rows computed rows is built;
 * *out stays NULL (status LS_OK) when even min_depth does not fit. Arrays: table (n_patches x 20 int32: own_start, n_own, n_rows,
 * n_local, W, off_gid, off_cols, off_diag, lim[12]), ghost_gid, cols16 ((W, n_rows) per patch), diag, perm (new -> old, V). */
typedef struct ls_patch_plan ls_patch_plan;
int ls_patch_plan_create(int64_t V, const int32_t* h_rowptr, const int32_t* h_col, const float* h_diag, const float* h_positions,
                         int patch_size, int depth, int cap_local, int min_depth, int cap_rows, ls_patch_plan** out);
int ls_patch_plan_destroy(ls_patch_plan* p);
int ls_patch_plan_info(const ls_patch_plan* p, int* n_patches, int* depth, int* max_local, int* max_rows, int* max_width, int64_t* n_gid,
                       int64_t* n_cols, int64_t* n_diag, double* seconds);
int ls_patch_plan_arrays(const ls_patch_plan* p, int32_t* table, int32_t* ghost_gid, uint16_t* cols16, float* diag, int32_t* perm);

/* ---- host-side analysis of a vertex-block shard of the iterative solvers (csrc/shard_plan.cpp; one process per GPU, halo exchange):
 * rank `rank` of P owns the rows [rank V / P, (rank + 1) V / P) of the CSR matrix (h_rowptr, h_col, h_val); with depth s it also computes
 * the ghost layers 1..s-1 redundantly and reads layer s. Local column ids: [owned | computed ghosts | read-only ghosts], each ghost group
 * sorted by global id. Arrays: local rowptr (n_own + n_inner + 1) / col / val (n_entries), ghosts (global ids, n_ghosts), recv3 (n_recv x
 * {source rank, offset in the ghost region, count}), send lists as CSR: send_ptr (n_send + 1), send_dst (n_send), send_ids (owned-row
 * indices, message for message in the RECEIVER's order). ls_shard_layer_sizes: sizes of the ghost layers 1..depth of a block [lo, hi). */
typedef struct ls_shard_plan ls_shard_plan;
int ls_shard_plan_create(int64_t V, const int32_t* h_rowptr, const int32_t* h_col, const float* h_val, int P, int rank, int depth,
                         ls_shard_plan** out);
int ls_shard_plan_destroy(ls_shard_plan* s);
int ls_shard_plan_info(const ls_shard_plan* s, int64_t* lo, int64_t* hi, int64_t* n_inner, int64_t* n_ghosts, int64_t* n_entries,
                       int* n_recv, int* n_send, int64_t* n_send_ids);
int ls_shard_plan_arrays(const ls_shard_plan* s, int32_t* rowptr, int32_t* col, float* val, int32_t* ghosts, int32_t* recv3,
                         int32_t* send_ptr, int32_t* send_dst, int32_t* send_ids);
int ls_shard_layer_sizes(int64_t V, const int32_t* h_rowptr, const int32_t* h_col, int64_t lo, int64_t hi, int depth, int64_t* h_sizes);

/* Symbolic analysis alone, on the HOST (no device is touched): the elimination tree and everything static of the solver above
 * for the CSR pattern (h_rowptr, h_col; structurally symmetric) of a V x V matrix. h_positions: (V, 3) vertex positions the
 * geometric bisection runs on (only their spatial order matters), or NULL: graph-distance pseudo-positions are derived from
 * the pattern. smooth: neighbour-averaging passes applied to the positions first (4 is the solver's default). */
typedef struct ls_nd_plan ls_nd_plan;
int ls_nd_plan_create(int64_t V, const int32_t* h_rowptr, const int32_t* h_col, const float* h_positions, int leaf_size,
                      int arity, int smooth, ls_nd_plan** out);
/* The same plan as ls_direct_factor forms it: the positions' smoothing and the bisection rounds run ON THE DEVICE (csrc/nd_bisect.hip:
 * three coordinate orders by radix sort, a stable partition per round), the rest on the host. d_positions may be NULL. Bit-identical
 * to ls_nd_plan_create on the same input -- the GPU tests compare the two. SYNC. */
int ls_nd_plan_create_device(const int32_t* d_rowptr, const int32_t* d_col, const float* d_positions, int64_t V, int64_t nnz,
                             int leaf_size, int arity, int smooth, int device, void* stream, ls_nd_plan** out);
/* How the cutting direction of a domain is chosen (replaces the graph-based fill-reducing ordering CHOLMOD runs behind the reference's
 * constructor, largesteps/solvers.py:34 -- which does not depend on how the surface lies in space):
 *   LS_ND_ORDER_LONGEST (0)  median cut along the longest axis of the domain's bounding box in the embedding (positions, or graph
 *                            distances without positions) -- what ls_nd_plan_create / ls_nd_plan_create_device run;
 *   LS_ND_ORDER_MINSEP  (1)  every domain tries the three position axes AND three graph distances and takes the thinnest separator
 *                            (host threads): a surface that is folded or rolled up in space, or shells inside each other, dissect
 *                            like the flat sheet (a cutting plane crosses every layer, a level set of a graph distance crosses one);
 *   LS_ND_ORDER_AUTO   (-1)  LONGEST first; if its separators are thicker than a surface's should be (spread > 1.3, below), MINSEP
 *                            too, and the plan with fewer factor numbers -- what ls_direct_factor runs (environment LS_ND_ORDER
 *                            overrides, LS_ND_SUSPECT moves the threshold).
 * ls_nd_plan_quality / ls_direct_plan_quality: the rule that built the plan, factor numbers per vertex (sum over the nodes of
 * s^2 + 2 s b, / V), spread = sum of s^2 over the inner nodes / (A x sum of their subtrees' vertex counts) with A = (sum_{j < log2
 * arity} 2^(j/2))^2 -- ~0.7 on a flat sheet at ANY size, 1.0-1.2 on closed surfaces, 1.4 on a sheet folded once, 5-75 on scrolls --,
 * and the factor numbers per vertex of the plan AUTO built and did not take (0: it built one). Any pointer may be NULL. Host only. */
#define LS_ND_ORDER_AUTO (-1)
#define LS_ND_ORDER_LONGEST 0
#define LS_ND_ORDER_MINSEP 1
int ls_nd_plan_create_ordered(int64_t V, const int32_t* h_rowptr, const int32_t* h_col, const float* h_positions, int leaf_size,
                              int arity, int smooth, int ordering, ls_nd_plan** out);
/* ls_nd_plan_create_device with the ordering rule as an argument: LS_ND_ORDER_MINSEP runs the trial cuts ON THE DEVICE (six sorted lists, a
 * side bit and a cut bit per vertex and direction; the graph distances are breadth-first sweeps on the host) and is bit-identical to
 * ls_nd_plan_create_ordered(..., LS_ND_ORDER_MINSEP) on the same input; LS_ND_ORDER_AUTO is what ls_direct_factor runs. SYNC. */
int ls_nd_plan_create_device_ordered(const int32_t* d_rowptr, const int32_t* d_col, const float* d_positions, int64_t V, int64_t nnz,
                                     int leaf_size, int arity, int smooth, int ordering, int device, void* stream, ls_nd_plan** out);
int ls_nd_plan_quality(const ls_nd_plan* p, int* h_ordering, double* h_words_per_vertex, double* h_spread, double* h_words_other);
int ls_nd_plan_destroy(ls_nd_plan* p);
int ls_nd_plan_info(const ls_nd_plan* p, int* levels, int* arity, int* n_nodes, int64_t* n_bnd, int64_t* n_front, double* seconds);
/* copies out: perm (V), s / b / own_start / parent (n_nodes + 1 each, node ids are 1-based), bnd / ppos / push_tgt (n_bnd),
 * push_ptr (n_front + 1); any pointer may be NULL */
int ls_nd_plan_arrays(const ls_nd_plan* p, int32_t* perm, int32_t* s, int32_t* b, int32_t* own_start, int32_t* parent,
                      int32_t* bnd, int32_t* ppos, int32_t* push_ptr, int32_t* push_tgt);

typedef struct ls_direct ls_direct;
/* The plan and the factor of one matrix, as plain arrays. h_* live on the host and are copied; d_* are DEVICE arrays
 * owned by the caller and kept alive for the handle's lifetime.
 * h_nodes: (n_nodes + 1, LS_DIRECT_NODE_COLS) int64, row i = {s, b, own_start, bnd_off, front_off, finv_off, w_off, parent,
 *          tri_off, spb_off, sps_off, quad} (row 0 unused). The deepest levels may be stored in the layouts of the tier
 *          kernels (csrc/nd_tier.h), which then run them as ONE launch per sweep, a workgroup per subtree:
 *          quad != 0: a dense node whose two matrix streams are quad-interleaved along the reduction (a lane reads 16 bytes
 *              = 4 consecutive reduction entries; reductions padded to multiples of 4 with zeros; s4 = s rounded up to 4):
 *              d_u4[w_off + ((j / 4) * b + i) * 4 + j % 4] = W[i][j]                                        (up sweep)
 *              d_d4[finv_off + ((t / 4) * s + j) * 4 + t % 4] = [F_ss^-1 (padded to s4 columns) | W^T][j][t]  (down sweep)
 *              (finv_off, w_off multiples of 4 floats);
 *          tri_off >= 0: a SPARSE LEAF (last level, 1 <= s <= 64; all leaves with s >= 1 alike): instead of dense arrays
 *              it owns  d_tri[tri_off + r (r + 1) / 2 + c] = (F_ss^-1)[r][c], c <= r  (packed rows of the lower triangle,
 *              tri_off a multiple of 4 floats), and its off-diagonal block A_bs of the matrix itself as two CSR lists in
 *              d_sp_ptr / d_sp_ent: boundary row i owns the entries d_sp_ptr[spb_off + i] .. d_sp_ptr[spb_off + i + 1]
 *              ({value, own-row index}), own row j the entries d_sp_ptr[sps_off + j] .. [sps_off + j + 1] ({value, boundary
 *              index}). Up sweep  y = F_ss^-1 b_s, update = A_bs y;  down sweep  x_s = y - F_ss^-1 (A_sb x_bnd).
 *          Tier-layout levels must be the deepest ones, complete levels, at most 6 of them. */
#define LS_DIRECT_NODE_COLS 12
typedef struct ls_direct_arrays {
    int64_t V;
    int32_t levels, arity;
    const int64_t* h_nodes;
    const int32_t* h_perm;
    const int32_t* h_ppos;
    int64_t n_bnd;
    const int32_t* h_push_ptr;
    const int32_t* h_push_tgt;
    int64_t n_front;
    const float* d_finv;
    const float* d_wf;
    const float* d_wb;
    const float* d_u4;
    const float* d_d4;
    const float* d_tri;
    const int32_t* d_sp_ptr;
    const void* d_sp_ent;          /* {float value; int32 index} pairs */
    int64_t n_sp_ptr, n_sp_ent;    /* lengths of the two sparse-leaf arrays (accounting only) */
    int32_t shard_rank, shard_count;   /* subtree sharding over `shard_count` processes (0 or 1: none), see ls_direct_solve_part */
    int32_t tier_waves;                /* waves per tier workgroup: 0 = the library's rule (see ls_direct_options), 4 / 8 / 16; else LS_E_INVALID */
} ls_direct_arrays;
int ls_direct_create(const ls_direct_arrays* arrays, int device, void* stream, ls_direct** out);
/* The tree ls_direct_factor picks for a V x V system: on entry *leaf_size / *arity <= 0 mean "pick" (explicit values are kept), on return
 * both hold what the factorisation will use. Host only (no device is touched): the rule is a table of measured crossovers
 * (profiles/r03_leaf_size_sweep.txt), documented in DESIGN.md section 2.3 (table: docs/history_rounds_1_4.md). */
int ls_direct_pick_tree(int64_t V, int* leaf_size, int* arity);
/* Host only: the dynamic LDS (bytes) one workgroup of the tier kernels needs to walk a subtree of the `tier_levels` deepest levels of a plan
 * (h_s / h_b / h_own_start: per node id, 1-based, level-major -- what ls_nd_plan_arrays returns), with `waves` = 4, 8 or 16 waves per workgroup;
 * 0 = such a tier cannot be planned (a level mixing sparse and dense leaves). ls_direct_factor takes the 16-wave tier only while this is <= 160 KB
 * and the 4-wave one while it is <= 150 KB. sparse_leaves != 0: leaves of at most 64 rows are stored as triangle + sparse block. */
int ls_direct_tier_lds_bytes(int levels, int arity, const int32_t* h_s, const int32_t* h_b, const int32_t* h_own_start, int tier_levels,
                             int sparse_leaves, int waves, size_t* h_bytes);
/* Matrix in, solver out: symbolic analysis (bisection rounds on the device, csrc/nd_bisect.hip; tree, fronts and index lists on
 * host threads), numeric multifrontal factorisation in fp64 on the device with hand-written kernels (csrc/nd_factor.hip: products
 * on the fp64 matrix instruction, SPD inverses in registers), fp32 factor in the solve kernels' layouts, handle. This one call is the
 * constructor of the reference's default solver (largesteps/solvers.py:34, CholeskySolverF(n, ii, jj, x, MatrixType.COO)).
 * d_rowptr / d_col / d_val: CSR of the symmetric positive definite matrix (DEVICE, original numbering, column-sorted rows);
 * d_positions: (V, 3) fp32 vertex positions (DEVICE) or NULL (graph-distance pseudo-positions);
 * arity 2 / 4 / 8 = children per tree node (1 / 2 / 3 bisection rounds per level) and leaf_size = the largest leaf, or <= 0 = chosen
 *   by the library from V (ls_direct_pick_tree above; small and medium systems are bound by their chain of launches, not by bytes):
 *   one dense node up to 1280 unknowns (ONE launch per re-solve), arity 4 with leaves of up to 1024 up to 12k, arity 8 between 12k and
 *   300k (three levels of dense nodes up to 36k, four levels with dense leaves of 70-205 rows up to 105k, five levels with 64-vertex
 *   sparse leaves beyond), arity 4 with 64-vertex sparse leaves -- the large-mesh setting -- above 300k;
 * tier_levels deepest levels go into the tier layouts (-1 = chosen by the library: tree levels - 5, at least 2 and at most 4; from
 *   800k unknowns on an arity-4 tree of at least 8 levels, one GPU: tree levels - 4, walked by one 16-wave workgroup per CU; the leaf
 *   level alone for many dense leaves of 65-224 rows in a tree of at most 4 levels; none for leaves of more than 256 rows or a single
 *   node; 0 = none); sparse_leaves != 0 stores leaves of at most 64 rows as packed triangle + sparse block;
 * shard_rank / shard_count: subtree sharding (0 / 1: none; every rank factorises the whole matrix, the re-solve is sharded, see
 *   ls_direct_solve_part).
 * The host half of the analysis runs on a pool of threads (environment LS_PLAN_THREADS, default 32, at most the host's cores divided
 * by LOCAL_WORLD_SIZE) that is created by the first call and kept, asleep, for the life of the process; a call made while another
 * thread's call holds the pool, or from a forked child, uses threads of its own.
 * SYNC. Errors: LS_E_INVALID (not symmetric / not positive definite / bad arguments), LS_E_WORKSPACE (fronts or factor beyond the
 * solver's limits; or an EXPLICIT tier_levels whose subtrees do not fit a workgroup's LDS -- tier_levels = -1 lowers its own choice
 * until it fits and never fails for that reason). */
int ls_direct_factor(const int32_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t V, int64_t nnz,
                     const float* d_positions, int leaf_size, int arity, int tier_levels, int sparse_leaves, int shard_rank,
                     int shard_count, int device, void* stream, ls_direct** out);
/* The same constructor with every choice as an argument (round 6; `ordering` used to reach the library through the process
 * environment only). Fill the struct with ls_direct_options_default, change what you need:
 *   leaf_size, arity, tier_levels, sparse_leaves, shard_rank, shard_count: as ls_direct_factor's arguments (defaults 0, 0, -1, 1, 0, 1);
 *   ordering    how the bisection picks its cutting directions: LS_ND_ORDER_AUTO (the library's rule: trial cuts where the separators
 *               are thicker than a surface's should be), LS_ND_ORDER_LONGEST, LS_ND_ORDER_MINSEP (trial cuts always: 5-10 % fewer factor
 *               numbers on rough closed scans for 10-25 ms more constructor). An explicit value wins; AUTO lets the environment
 *               variable LS_ND_ORDER override the rule (A/B runs);
 *   tier_waves  waves per workgroup of the tier kernels: 0 = the library's rule (16 on one workgroup per CU and a subtree one level
 *               taller from 800k unknowns, 8 for <= 768 subtrees, 4 otherwise), or 4 / 8 / 16. An explicit value wins; 0 lets
 *               LS_ND_TIER_WAVES override.
 * struct_bytes = sizeof(ls_direct_options) of the CALLER's header: fields a newer library knows beyond it take their defaults.
 * opt == NULL: all defaults (= ls_direct_factor(..., 0, 0, -1, 1, 0, 1, ...)). */
typedef struct ls_direct_options {
    int32_t struct_bytes;
    int32_t leaf_size, arity, tier_levels, sparse_leaves, shard_rank, shard_count;
    int32_t ordering;
    int32_t tier_waves;
} ls_direct_options;
int ls_direct_options_default(ls_direct_options* opt);
int ls_direct_factor_ex(const int32_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t V, int64_t nnz,
                        const float* d_positions, const ls_direct_options* opt, int device, void* stream, ls_direct** out);
/* Same-pattern refactorisation: new values, same sparsity pattern, no new symbolic analysis.
 * ls_direct_factor_refactorable: exactly ls_direct_factor_ex (same plan, same layouts, bit-identical solves), but the handle also keeps
 *   what a numeric refactorisation needs -- a device copy of the analysed pattern (rowptr, col), the tree's index lists and node table,
 *   the recorded chain of numeric launches (its descriptors as offsets into the scratch, not pointers) and, with sparse leaves, where
 *   every stored entry's value lives in their lists (8 bytes per entry). ~120 MB at 1M vertices (profiles/refactor_bench.json); the fp64 scratch (3-4 GB) is NOT kept.
 *   A sharded handle (shard_count > 1) keeps nothing. SYNC.
 * ls_direct_refactor: SYNC. The caller's pattern is compared with the kept one on the device (one flag read back): V, nnz, rowptr or col
 *   different -> LS_E_INVALID, the factor untouched. Otherwise scratch comes from the buffer pool, the KEPT pattern plus the caller's values
 *   are assembled (no caller array steers a write), the constructor's numeric chain runs into the handle's own factor arrays in place,
 *   and the scratch goes back to the pool. The result is bitwise what ls_direct_factor_ex(new values) with the same positions and
 *   options would give. No buffer a solve reads or writes moves: a graph captured around solves of this handle replays with the new
 *   factor. A front that is not positive definite -> LS_E_INVALID and the handle is UNFACTORED (ls_direct_solve / _solve_part return
 *   LS_E_STATE) until a later ls_direct_refactor succeeds. LS_E_STATE: the handle was not made by ls_direct_factor_refactorable (or is
 *   sharded), or `stream` is being captured (the call synchronises).
 * ls_direct_refactorable: host only; *h_yes = 1 if ls_direct_refactor can run on the handle, *h_retained_device_bytes = what it keeps
 *   for that (either pointer may be NULL). */
int ls_direct_factor_refactorable(const int32_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t V, int64_t nnz,
                                  const float* d_positions, const ls_direct_options* opt, int device, void* stream, ls_direct** out);
int ls_direct_refactor(ls_direct* d, const int32_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t V, int64_t nnz,
                       void* stream);
int ls_direct_refactorable(const ls_direct* d, int* h_yes, size_t* h_retained_device_bytes);
/* The direct solver keeps its device buffers (>= 256 KB: the constructor's fp64 fronts and work arrays -- 3-4 GB at 1M vertices, 14 GB
 * at 4M --, the analysis' scratch, a destroyed handle's factor arrays, index tables and vectors) in a per-process pool instead of freeing them: a remesh loop
 * (scripts/main.py:137-169) destroys a solver and constructs one of nearly the same size again and again, and the runtime gives freed
 * memory back lazily -- at the 4M size every second or third construction stalled 0.45-0.7 s inside one hipMalloc. The pool holds at most
 * LS_POOL_GB per device (environment, default 24; 0 = no pool; oldest out first) and never more than a quarter of the device's memory. An
 * allocation of the library that fails for lack of memory empties the pool of its device and is repeated once. This call frees what the
 * pool holds (device < 0: on every device) -- for callers whose OWN allocator ran out (torch's caching allocator cannot see the pool). */
int ls_release_scratch(int device);
/* tree levels, arity, levels run by the tier kernels and their workgroup count, 4-byte words of factor data the up / the
 * down sweep reads, total boundary entries (any pointer may be NULL) */
int ls_direct_shape(const ls_direct* d, int* h_levels, int* h_arity, int* h_tier_levels, int* h_tier_workgroups,
                    int64_t* h_words_up, int64_t* h_words_down, int64_t* h_n_bnd);
/* 4-byte words of factor data each tree level reads in the up / the down sweep (h_up, h_down: `cap` entries, level 0 = root;
 * the sparse leaves' lists are counted with the last level). Host only. */
int ls_direct_level_words(const ls_direct* d, int cap, int64_t* h_up, int64_t* h_down);
/* own rows (vertices) and boundary entries of each tree level (level 0 = root): what the vectors a level's launch moves are made
 * of -- per sweep b / b' / x rows of its vertices and the boundary vectors of its nodes. Host only. */
int ls_direct_level_rows(const ls_direct* d, int cap, int64_t* h_rows, int64_t* h_bnd);
/* bytes of STATIC index data each tree level's launch reads per sweep, besides the factor words (ls_direct_level_words) and the vectors
 * (ls_direct_level_rows): tile / item records, children masks, parent positions, the tier's pull lists (arity indices per front position
 * of an inner node), push-list pointers and targets. perm (4 bytes per own row and sweep) is counted with the vectors. Host only. */
int ls_direct_level_index_bytes(const ls_direct* d, int cap, int64_t* h_up, int64_t* h_down);
/* how evenly the tier's subtrees (one workgroup each) are loaded: h_words4 = {max, mean} factor words of a subtree in the up sweep,
 * {max, mean} in the down sweep. With one workgroup per CU the heaviest subtree is the launch's time. Zeros without a tier. Host only. */
int ls_direct_tier_balance(const ls_direct* d, double* h_words4);
/* After a solve with "profile" = 3 (an event in front of every launch; the solve synchronises): number of launches and, for
 * the first `cap` of them, duration in ms, factor words read, tree levels [lo, hi] covered, sweep (0 up, 1 down, 2 both).
 * Any pointer may be NULL. */
int ls_direct_launch_profile(const ls_direct* d, int cap, int* h_n, double* h_ms, int64_t* h_words, int32_t* h_level_lo,
                             int32_t* h_level_hi, int32_t* h_sweep);
/* the dissection behind a handle made by ls_direct_factor (see ls_nd_plan_quality) */
int ls_direct_plan_quality(const ls_direct* d, int* h_ordering, double* h_words_per_vertex, double* h_spread, double* h_words_other);
/* seconds of the three constructor stages of a handle made by ls_direct_factor: symbolic analysis, layout tables, numeric */
int ls_direct_factor_seconds(const ls_direct* d, double* h_s3);
/* SYNC: *h_symmetric = 1 iff every stored entry (r, c, v) has a stored mirror (c, r, v') with |v - v'| <= tol */
int ls_csr_is_symmetric(const int32_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t V, int64_t nnz, float tol,
                        int* h_symmetric, int device, void* stream);
int ls_direct_destroy(ls_direct* d);
/* x = M^-1 b for k <= 4 interleaved columns ((V, k) row-major, b != x) */
int ls_direct_solve(ls_direct* d, const float* b, float* x, int k, void* stream);
/* Subtree sharding, one process per GPU (largesteps/distributed.py ShardedDirect): a handle created with shard_count = N > 1
 * runs the subtrees of the first tree level that has >= N of them ("cut" level; rank r takes a contiguous share) and,
 * replicated on every rank, the levels above the cut. One solve =
 *     part 0   this rank's subtrees upwards; their updates for level cut - 1 land in `exchange` (floats_per_column x k floats,
 *              zero where another rank's subtree contributes)
 *     the caller SUMS `exchange` over the ranks (one all-reduce of a few hundred KB; every entry has exactly one non-zero
 *     contributor, so the sum is exact and order independent)
 *     part 1   the replicated levels up and down, then this rank's subtrees downwards: x rows of the rank's subtrees and of
 *              the replicated levels are written, other rows of x are left untouched.
 * h_owned_rows (V bytes, may be NULL): 1 where this rank is the designated owner of the row (replicated levels: rank 0). */
int ls_direct_solve_part(ls_direct* d, const float* b, float* x, int k, int part, float* exchange, void* stream);
int ls_direct_shard_info(const ls_direct* d, int* h_rank, int* h_count, int* h_cut_level, int64_t* h_exchange_floats_per_column,
                         unsigned char* h_owned_rows);
/* the region of the handle's own workspace that holds the exchange of a k-column solve (what part 0 leaves and part 1 reads):
 * passing it as `exchange` to ls_direct_solve_part skips the staging copies -- the caller then reduces it in place */
int ls_direct_exchange_region(ls_direct* d, int k, float** h_region, int64_t* h_floats);

/* ---- the collective of the sharded solve behind the C ABI (one process per GPU; RCCL over xGMI, looked up at run time) --------------
 * ls_dist_unique_id: rank 0 creates a 128-byte communicator id and ships it to the other ranks (any transport: the caller's);
 * ls_dist_create: COLLECTIVE, every rank calls it with the same id (ncclCommInitRank on `device`);
 * ls_dist_allreduce_sum: in-place sum of n floats over the ranks, ASYNC on `stream`;
 * ls_dist_direct_solve: one sharded solve = ls_direct_solve_part(0), the all-reduce of the exchange region in place, part (1),
 *   all on `stream` with no host round trip in between (a consumer needs no Python and no all-reduce of its own).
 * LS_E_STATE: librccl.so is not loadable; values >= 2000: 2000 + ncclResult_t. */
typedef struct ls_dist ls_dist;
int ls_dist_unique_id(void* h_id128);
int ls_dist_create(const void* h_id128, int rank, int world, int device, ls_dist** out);
int ls_dist_destroy(ls_dist* c);
int ls_dist_allreduce_sum(ls_dist* c, float* d_buf, int64_t n, void* stream);
/* what the RCCL communicator itself reports (ncclCommUserRank / ncclCommCount), not what the caller passed to ls_dist_create */
int ls_dist_info(const ls_dist* c, int* h_rank, int* h_world);
int ls_dist_direct_solve(ls_dist* c, ls_direct* d, const float* b, float* x, int k, void* stream);
/* knobs: "profile" (1: the next solves time the up sweep and the down sweep with HIP events and synchronise; 3: an event in
 * front of every launch, read back by ls_direct_launch_profile);
 * "nt" (cache policy of the read-once factor streams: 1 non-temporal loads, 0 default policy, -1 the library's rule -- non-temporal
 * once the factor exceeds what the 256 MB Infinity Cache keeps from solve to solve; results are bit-identical either way) */
int ls_direct_set(ls_direct* d, const char* name, int value);
/* host-only: 4-byte words of factor data one solve reads, kernel launches per solve, {up sweep, down sweep, 0} ms of the
 * last profiled solve (any pointer may be NULL) */
int ls_direct_info(const ls_direct* d, int64_t* h_factor_entries, int* h_launches, double* h_ms3);

/* ---- remove_duplicates (reference scripts/geometry.py:3-11) --------------------------------------
 * unique_verts = the distinct rows of verts ((V, 3) fp32) in lexicographic order of their VALUES (-0.0 == 0.0), exactly what
 * torch.unique(v, dim=0, return_inverse=True) returns; inverse (V) int64: verts[i] == unique_verts[inverse[i]];
 * new_faces (F, 3) int64 = inverse[faces] (faces int32 / int64 by idx_bytes; F may be 0). unique_verts needs room for V rows;
 * *h_n_unique receives the number of rows written. Hand-written stable LSD radix sort (no library sort). SYNC.
 * A face index outside [0, V) -> LS_E_INDEX. */
int ls_remove_duplicates_workspace_bytes(int64_t V, size_t* h_bytes);
int ls_remove_duplicates(const float* verts, int64_t V, const void* faces, int idx_bytes, int64_t F, float* unique_verts,
                         int64_t* inverse, int64_t* new_faces, int64_t* h_n_unique, void* workspace, size_t ws_bytes, int device,
                         void* stream);

/* CSR of the transpose (rows of M^T sorted by column = original row), for the backward pass of to_differential on a matrix
 * that is not symmetric. Hand-written radix sort of the entry ids by column. SYNC (range check of the column indices). */
int ls_csr_transpose_workspace_bytes(int64_t V, int64_t nnz, size_t* h_bytes);
int ls_csr_transpose(const int32_t* rowptr, const int32_t* col, const float* val, int64_t V, int64_t nnz, int32_t* t_rowptr,
                     int32_t* t_col, float* t_val, void* workspace, size_t ws_bytes, int device, void* stream);
/* Vertex-major ranking of the 3 F face corners (see the normals below): vptr (V + 1) = first rank of every vertex, cpos (3 F) =
 * rank of corner 3 f + i; the corners of a vertex are ranked in ascending corner id. A face index outside [0, V) -> LS_E_INDEX.
 * SYNC. */
int ls_corner_ranks_workspace_bytes(int64_t F, int64_t V, size_t* h_bytes);
int ls_corner_ranks(const void* faces, int idx_bytes, int64_t F, int64_t V, int32_t* vptr, int32_t* cpos, void* workspace,
                    size_t ws_bytes, int device, void* stream);

/* ---- normals ----------------------------------------------------------------------
 * faces: (F, 3) int32 or int64 (idx_bytes 4 / 8), verts (V, 3) fp32. Face normals are (3, F) like the reference returns
 * them. Semantics of scripts/geometry.py kept to the letter: a degenerate face / an unreferenced vertex gives NaN, and
 * the corner "angles" are acos(clamp(e_a . e_b / (||E_a||_F ||E_b||_F))) with the FROBENIUS norms of the whole edge
 * matrices (geometry.py:138-141), not per-face lengths. Indices are not range checked (the host wrapper does that).
 * vptr (V + 1) / cpos (3 F): corner 3 f + i has rank cpos[3 f + i] in the vertex-major order of all corners and vertex
 * v owns the ranks [vptr[v], vptr[v + 1]); the per-face kernels store one vector per corner at its rank and a
 * per-vertex kernel sums its contiguous range in rank order -- no atomics, bitwise reproducible for a given ranking. */
int ls_normals_workspace_bytes(int64_t F, int64_t V, size_t* h_bytes);
int ls_face_normals(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, float* fn, int device, void* stream);
/* grad_verts (V, 3) = d sum(g_fn * fn) / d verts; overwritten */
int ls_face_normals_backward(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                             const int32_t* cpos, const float* g_fn, float* grad_verts, void* workspace, size_t ws_bytes,
                             int device, void* stream);
/* out (V, 3) normalised vertex normals; raw (V, 3) the unnormalised sums and norms[3] = {||E01||, ||E02||, ||E12||} are
 * kept by the caller for the backward pass */
int ls_vertex_normals(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                      const int32_t* cpos, const float* fn, float* out, float* raw, float* norms, void* workspace,
                      size_t ws_bytes, int device, void* stream);
/* grad_verts (V, 3) and grad_fn (3, F) of sum(g_out * out) with the face normals an independent input; both overwritten */
int ls_vertex_normals_backward(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                               const int32_t* cpos, const float* fn, const float* raw, const float* norms, const float* g_out,
                               float* grad_verts, float* grad_fn, void* workspace, size_t ws_bytes, int device, void* stream);
/* The PAIR compute_face_normals -> compute_vertex_normals on one mesh (scripts/main.py:178-179: the face normals handed to
 * compute_vertex_normals ARE the normalised cross products of the same vertices). Then the two are one function of the
 * vertices and the passes share work: the face-normal pass also reduces the three edge norms, later passes recompute n_f from
 * the positions they load anyway instead of reading (3, F), and the backward stores the corner buffer once:
 *   forward    ls_face_normals_with_norms (fn, norms[3])  ->  ls_vertex_normals_from_norms (out, raw)
 *   backward   ls_normals_pair_backward_faces: g_raw (V, 3) = gradient of the unnormalised sums, gN[3] = dL/d(edge norms),
 *              grad_fn (3, F) = what reaches the face normals through the vertex normals -- an OUTPUT of the pair, the
 *              caller adds what other consumers of the face normals contribute -- then
 *              ls_normals_pair_backward_verts: grad_verts (V, 3) of everything, g_fn = that total (nullptr: none).
 * Same values as the separate calls up to the order of a few additions. g_raw / gN are the caller's (they live between the
 * two backward calls); workspace as above.
 * ls_vertex_normals_gathered = ls_vertex_normals_from_norms bit for bit, vertex-major: a thread per vertex walks its corners in
 * rank order and recomputes their contributions (no corner buffer, no workspace, one launch instead of two: 32 against 46 us at
 * 1M vertices). order[3 F] is the inverse permutation of cpos (order[cpos[c]] = c: rank -> corner id 3 f + i).
 * PRECONDITION of ls_vertex_normals_gathered (NOT checked on the device, unlike ls_corner_ranks / ls_assemble_*, which validate and
 * return LS_E_INDEX): vptr / order must be what ls_corner_ranks returned FOR THESE faces, i.e. every face index lies in [0, V) and
 * every order entry in [0, 3 F) -- the kernel indexes verts through them without a range check. */
int ls_face_normals_with_norms(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, float* fn, float* norms,
                               void* workspace, size_t ws_bytes, int device, void* stream);
int ls_vertex_normals_from_norms(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                                 const int32_t* cpos, const float* norms, float* out, float* raw, void* workspace, size_t ws_bytes,
                                 int device, void* stream);
int ls_vertex_normals_gathered(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                               const int32_t* order, const float* norms, float* out, float* raw, int device, void* stream);
int ls_normals_pair_backward_faces(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const float* raw,
                                   const float* norms, const float* g_out, float* g_raw, float* gN, float* grad_fn, void* workspace,
                                   size_t ws_bytes, int device, void* stream);
int ls_normals_pair_backward_verts(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                                   const int32_t* cpos, const float* norms, const float* g_raw, const float* gN, const float* g_fn,
                                   float* grad_verts, void* workspace, size_t ws_bytes, int device, void* stream);

/* ---- meshgeom: average_edge_length and massmatrix_voronoi ------------------------------------------------------
 * faces (F, 3) int32 / int64 (idx_bytes 4 / 8), verts (V, 3) fp32, vptr / cpos / order the corner ranking of ls_corner_ranks
 * (order[3 F] = its inverse permutation, rank -> corner id 3 f + i), as for the normals above. Same PRECONDITION as
 * ls_vertex_normals_gathered: the ranking was built FOR THESE faces (ls_corner_ranks has range-checked them and returns
 * LS_E_INDEX otherwise); the kernels index verts through faces / order without a range check. No entry point allocates or
 * synchronises; no atomics -- every result is bitwise reproducible for a given ranking. ASYNC.
 *   ls_massmatrix_voronoi      mass (V) fp32: the reference's per-face cells in its fp32 operation order, summed per vertex as its
 *                              scatter_add_ + sum(dim=1) does (per corner slot j in ascending face id, then (s0 + s1) + s2);
 *                              vertex-major, one launch, no workspace. Unreferenced vertex: 0; a face with a zero-length edge: NaN.
 *   ls_massmatrix_voronoi_backward   grad_verts (V, 3) = d sum(g_mass * mass) / d verts (torch's backward rules), overwritten.
 *   ls_average_edge_length     out[0] = (sum over faces of l0 + l1 + l2) / F / 3 (fp64 partial sums in a fixed order, the two
 *                              divisions in fp32 as the reference writes them); F == 0: NaN. Needs no ranking.
 *   ls_average_edge_length_backward  grad_verts (V, 3) = g_out[0] * d out / d verts; g_out is read on the device, overwritten. */
int ls_meshgeom_workspace_bytes(int64_t F, int64_t V, size_t* h_bytes);
int ls_massmatrix_voronoi(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                          const int32_t* order, float* mass, int device, void* stream);
int ls_massmatrix_voronoi_backward(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                                   const int32_t* cpos, const float* g_mass, float* grad_verts, void* workspace, size_t ws_bytes,
                                   int device, void* stream);
int ls_average_edge_length(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, float* out, void* workspace,
                           size_t ws_bytes, int device, void* stream);
int ls_average_edge_length_backward(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                                    const int32_t* cpos, const float* g_out, float* grad_verts, void* workspace, size_t ws_bytes,
                                    int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Botsch-Kobbelt isotropic remeshing (scripts/main.py:149 calls remesh_botsch(v, f, 5, h, True) of an external CPU build):
 * one iteration = split -> collapse -> flip -> relax -> project, fp32, every phase in rounds of conflict-free operations
 * ("Isotropic remeshing"; tests/remesh_statement.py states every rule). The output is bitwise reproducible: no float
 * atomics, ties broken by (value, edge id), new ids from exclusive scans. The output size is not known in advance, hence a handle:
 *   ls_remesh_create    copies verts (V, 3) fp32 and faces (F, 3) int32 / int64 (idx_bytes 4 / 8) of the device, checks that the
 *                       mesh is an edge-manifold, consistently oriented triangle mesh whose vertices' faces form one fan each
 *                       (LS_E_INVALID otherwise, LS_E_INDEX for an index outside [0, V)), drops unreferenced vertices and keeps
 *                       the result as the projection target. h > 0 is the target edge length (split above 4/3 h, collapse
 *                       below 4/5 h); project != 0: every iteration ends with the projection. Synchronises the stream.
 *   ls_remesh_run       `iterations` full iterations. Reads sizes on the host every round: not capturable. SYNC.
 *   ls_remesh_phase     ONE phase on the current mesh (LS_REMESH_SPLIT / COLLAPSE / FLIP: up to max_rounds rounds, fewer when a
 *                       round finds nothing to do; RELAX / PROJECT: one pass). For tests of each phase on its own. SYNC.
 *   ls_remesh_info      V, F of the current mesh; counters[6] = rounds of split, collapse, flip, then splits, collapses, flips
 *                       done (over all calls); seconds[5] = host wall time per phase (split, collapse, flip, relax, project).
 *   ls_remesh_copy_out  verts (V, 3) fp32 and faces (F, 3) int32 / int64, device buffers of the caller. ASYNC.
 *   ls_remesh_destroy   gives the handle's buffers back to the scratch pool (ls_release_scratch empties it).
 * --------------------------------------------------------------------------------------------- */
#define LS_REMESH_SPLIT 0
#define LS_REMESH_COLLAPSE 1
#define LS_REMESH_FLIP 2
#define LS_REMESH_RELAX 3
#define LS_REMESH_PROJECT 4
int ls_remesh_create(const float* verts, int64_t V, const void* faces, int idx_bytes, int64_t F, float h, int project, int device,
                     void* stream, void** handle);
int ls_remesh_run(void* handle, int iterations);
int ls_remesh_phase(void* handle, int phase, int max_rounds);
int ls_remesh_info(void* handle, int64_t* V, int64_t* F, int64_t* counters, double* seconds);
int ls_remesh_copy_out(void* handle, float* verts, void* faces, int idx_bytes);
int ls_remesh_destroy(void* handle);

/* ------------------------------------------------------------------------------------------------
 * Point-to-mesh squared distance (libigl's point_mesh_squared_distance and hausdorff, which figures/comparison/generate_data.py and
 * the notebooks call on every recorded step; largesteps/distance.py). The rules are stated in csrc/distance.hip and DESIGN.md
 * section 2.8, restated in numpy / torch by tests/distance_statement.py: fp64 arithmetic from the fp32 coordinates, a degenerate
 * triangle measured as its closest segment, ties of the squared distance to the lowest triangle id. Bitwise reproducible.
 *   ls_mesh_distance_create   copies verts (V, 3) fp32 and faces (F, 3) int32 / int64 (idx_bytes 4 / 8) of the device and builds the
 *                             LBVH over the faces. LS_E_INDEX for an index outside [0, V); LS_E_INVALID for F = 0, V = 0, a null
 *                             pointer or another idx_bytes. SYNC.
 *   ls_mesh_distance_query    for n query points P (n, 3) fp32: sqrD (n) fp64 squared distance to the nearest face, I (n) int64 its
 *                             face id, C (n, 3) fp64 the closest point. Any of the three may be NULL. ASYNC on `stream`.
 *   ls_mesh_distance_max      out_sqd[0] (fp64, device) = max over the n points of their squared distance (0 for n = 0). ASYNC.
 *   ls_mesh_distance_destroy  synchronises the device (queries may run on any stream), then gives the handle's buffer back to the
 *                             scratch pool (ls_release_scratch empties it). NULL is accepted.
 * The gradient of sqrD (no second derivatives). The closest point is C = sum_k w_k V[F[I, k]]; the weights w follow from the same
 * region / segment tests as C. With d = p - C and g the incoming gradient of sqrD: d/dp = 2 g d, d/dV[F[I, k]] = -2 g w_k d (C minimises
 * over the face, so no derivative of w enters; on a tie this is the subgradient of the face the tie rule chose). Every term is formed in
 * fp64 and rounded to fp32 once; the vertex gradient is summed without float atomics in one fixed order (points of a face in ascending
 * id, a vertex's corners in the rank order of ls_corner_ranks): bitwise reproducible, no host synchronisation, capturable.
 *   ls_mesh_distance_weights  W (n, 3) fp64 = the weights of point P[i] on face I[i] of the handle's mesh. I must come from
 *                             ls_mesh_distance_query on the same handle and positions; it is not range-checked on the host (that would
 *                             synchronise): an I outside [0, F) reads nothing and gives NaN weights. ASYNC.
 *   ls_mesh_distance_backward_workspace_bytes  the workspace of ls_mesh_distance_backward for n points and F faces.
 *   ls_mesh_distance_backward P, I, C as the query took and returned them, g (n) fp64 the gradient of sqrD; vptr (V + 1) and
 *                             corner_order (3 F) the ranking of ls_corner_ranks over the handle's faces (corner_order: rank -> corner,
 *                             the inverse of its cpos). gP (n, 3) fp32 and gV (V, 3) fp32 may each be NULL; I, vptr, corner_order and
 *                             the workspace are needed for gV only. A point whose I is outside [0, F) adds nothing to gV (I must come
 *                             from the query, as above). LS_E_INVALID for a null required pointer, LS_E_WORKSPACE for a workspace
 *                             below ls_mesh_distance_backward_workspace_bytes(n, F). ASYNC.
 *   ls_mesh_distance_update   new positions verts (V, 3) fp32 for the handle's faces: the bounds, the slack and the LBVH are rebuilt in
 *                             the handle's buffer (no allocation, no device synchronisation); afterwards the handle answers exactly as
 *                             a fresh one built from verts. Queries of the handle in flight on other streams must have finished. SYNC
 *                             (the stream is synchronised: the bounds come to the host).
 * --------------------------------------------------------------------------------------------- */
int ls_mesh_distance_create(const float* verts, int64_t V, const void* faces, int idx_bytes, int64_t F, int device, void* stream,
                            void** handle);
int ls_mesh_distance_query(void* handle, const float* P, int64_t n, double* sqrD, int64_t* I, double* C, void* stream);
int ls_mesh_distance_max(void* handle, const float* P, int64_t n, double* out_sqd, void* stream);
int ls_mesh_distance_destroy(void* handle);
int ls_mesh_distance_weights(void* handle, const float* P, int64_t n, const int64_t* I, double* W, void* stream);
int ls_mesh_distance_backward_workspace_bytes(int64_t n, int64_t F, size_t* bytes);
int ls_mesh_distance_backward(void* handle, const float* P, int64_t n, const int64_t* I, const double* C, const double* g,
                              const int32_t* vptr, const int32_t* corner_order, float* gP, float* gV, void* ws, size_t ws_bytes,
                              void* stream);
int ls_mesh_distance_update(void* handle, const float* verts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rays against the mesh of a mesh-distance handle (libigl's ray_mesh_intersect, and what ambient_occlusion is built from;
 * largesteps/raycast.py). The same handle answers distances and rays; ls_mesh_distance_update moves both. The rule is stated in
 * csrc/raycast.hip and DESIGN.md section 2.10, restated in numpy by tests/ray_statement.py, and the device answers with the same bits:
 * Woop, Benthin and Wald's watertight test in fp64 from the fp32 inputs; a hit needs tmin <= t <= tmax (both ends inclusive); the
 * closest hit is the accepted face of smallest t, the lowest id on equal t; edges and vertices count as hits, a zero-area face is never
 * hit, a direction with a non-finite component or all zero hits nothing. O, D (n, 3) fp32 origins and directions (D need not be unit:
 * t is in units of |D|); trange (n, 2) fp64 (tmin, tmax) per ray, or NULL for [0, +inf].
 *   ls_mesh_ray_closest   t (n) fp64, I (n) int64, W (n, 3) fp64 the barycentric weights of the hit on the corners of face I. A miss
 *                         is t = +inf, I = -1, W = 0. Any of the three may be NULL.
 *   ls_mesh_ray_any       hit (n) one byte per ray: 1 iff some face is accepted, which is I >= 0 of ls_mesh_ray_closest.
 * The gradient of t (first order, the face held fixed; no gradient of W or I). With n = (b - a) x (c - a) of the hit face and
 * q = n / (n . d): dt/do = -q, dt/dd = -t q, dt/dV[F[I, k]] = W[k] q, every term multiplied by the incoming gradient g in fp64 and rounded
 * to fp32 once; a ray whose I is outside [0, F) adds nothing and gets zeros. The vertex gradient is summed as the distance's is: rays of
 * a face in ascending id, a vertex's corners in the rank order of ls_corner_ranks, without float atomics: bitwise reproducible.
 *   ls_mesh_ray_backward_workspace_bytes  the workspace of ls_mesh_ray_backward for n rays and F faces.
 *   ls_mesh_ray_backward  O, D as the query took them, I, W, t as it returned them, g (n) fp64 the gradient of t; vptr (V + 1) and
 *                         corner_order (3 F) as for ls_mesh_distance_backward. gO, gD (n, 3) fp32 and gV (V, 3) fp32 may each be NULL;
 *                         W, vptr, corner_order and the workspace are needed for gV only.
 * LS_E_INVALID for a null required pointer or n < 0, LS_E_OVERFLOW at 2^31 rays, LS_E_WORKSPACE for a workspace below
 * ls_mesh_ray_backward_workspace_bytes(n, F); n = 0 is a no-op (gV is zeroed). No call allocates or synchronises: all ASYNC on `stream`.
 * Queries and gradients on different streams may overlap each other and the distance queries of the same handle (they only read it);
 * none may overlap ls_mesh_distance_update or ls_mesh_distance_destroy of that handle, and two calls that share a workspace must be
 * ordered.
 * --------------------------------------------------------------------------------------------- */
int ls_mesh_ray_closest(void* handle, const float* O, const float* D, int64_t n, const double* trange, double* t, int64_t* I, double* W,
                        void* stream);
int ls_mesh_ray_any(void* handle, const float* O, const float* D, int64_t n, const double* trange, unsigned char* hit, void* stream);
int ls_mesh_ray_backward_workspace_bytes(int64_t n, int64_t F, size_t* bytes);
int ls_mesh_ray_backward(void* handle, const float* O, const float* D, int64_t n, const int64_t* I, const double* W, const double* t,
                         const double* g, const int32_t* vptr, const int32_t* corner_order, float* gO, float* gD, float* gV, void* ws,
                         size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The generalized winding number of points against the mesh of a mesh-distance handle (libigl's winding_number and
 * fast_winding_number, and the sign of signed_distance; largesteps/distance.py). The rule is stated in csrc/winding.hip and DESIGN.md
 * section 2.11 and restated in numpy by tests/winding_statement.py: per face the van Oosterom-Strackee solid angle over 4 pi in fp64
 * from the fp32 inputs, 0 when its numerator is 0; per node of the handle's hierarchy the area-weighted centre p, a radius r and the
 * moments of a three-term far field. A query walks the hierarchy in pre-order and takes a node's far field when |q - p| > beta r, a
 * leaf's exact term otherwise, adding in visiting order: a result depends on (mesh, query, beta) alone. A query with a non-finite
 * component gives NaN.
 *   ls_mesh_winding_bytes    the size of the moment buffer of a mesh of F faces. The caller owns the buffer (8-byte aligned).
 *   ls_mesh_winding_prepare  fills the buffer from the handle's current positions and hierarchy; again after ls_mesh_distance_update.
 *   ls_mesh_winding_query    w (n) fp64 for P (n, 3) fp32, beta >= 1; beta = +inf is ls_mesh_winding_exact (moments may be NULL then).
 *   ls_mesh_winding_exact    w (n) fp64: the sum over all faces in ascending id, no hierarchy.
 *   ls_mesh_winding_arrays   copies to device arrays, each or NULL: left, right (F - 1), esc (2 F - 1), tri (F), box (2 F - 1, 6) fp32
 *                            and mom (2 F - 1, 36) fp64 -- per node p (3), r, N (3), Ar, C (9), T (18: row i, columns jk = 00 01 02
 *                            11 12 22), a pad. Internal node i of F - 1, leaf i at F - 1 + i holding face tri[i]. For the tests.
 * LS_E_INVALID for a null required pointer, n < 0 or beta < 1 (or NaN), LS_E_OVERFLOW at 2^31 points; n = 0 is a no-op. No call
 * allocates or synchronises: all ASYNC on `stream`. Queries only read the handle and the buffer; none may overlap
 * ls_mesh_winding_prepare of that buffer or ls_mesh_distance_update / ls_mesh_distance_destroy of that handle.
 * --------------------------------------------------------------------------------------------- */
int ls_mesh_winding_bytes(int64_t F, size_t* bytes);
int ls_mesh_winding_prepare(void* handle, void* moments, void* stream);
int ls_mesh_winding_query(void* handle, const void* moments, const float* P, int64_t n, double beta, double* w, void* stream);
int ls_mesh_winding_exact(void* handle, const float* P, int64_t n, double* w, void* stream);
int ls_mesh_winding_arrays(void* handle, const void* moments, int32_t* left, int32_t* right, int32_t* esc, int32_t* tri, float* box,
                           double* mom, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The self-intersections of the mesh of a mesh-distance handle (libigl's fast_find_self_intersections; largesteps/distance.py). The
 * rule is stated in csrc/selfx.hip and DESIGN.md section 2.12 and restated in numpy by tests/selfx_statement.py: a segment (p, q)
 * crosses a face iff the ray rule above, with o = p and d = q - p formed in fp64, accepts the face with 0 <= t <= 1 (edges and vertices
 * count, det == 0 never hits, d == 0 hits nothing). For faces f < g, s = the number of equal (corner of f, corner of g) index pairs
 * among the nine: s >= 2 is never reported; s == 1 is reported iff the edge of f opposite the shared corner crosses g or the edge of g
 * opposite it crosses f; s == 0 iff one of the three edges of f crosses g or one of the three edges of g crosses f. And a pair is
 * reported only if the corner boxes of f and g (the smallest and largest of the three fp32 corners per axis) are within 2 e of each other
 * on all three axes, e = 2^-40 x the largest |coordinate| of the vertices: apart on an axis iff lo_g - e > hi_f + e or
 * hi_g + e < lo_f - e in fp64, false on a NaN. A real crossing always passes this clause; it leaves out what the segment test accepts on
 * rounding alone between far-apart faces of an exactly flat sheet. Coplanar overlaps are not reported (det == 0; in a tilted plane
 * whose shear rounds, det is a rounding error and coplanar faces with near boxes can be); faces without a common index that touch at a
 * point or along a segment are.
 *   ls_mesh_selfx_count            counts (F) int32: counts[f] = the number of reported pairs (f, g) with g > f; total (int64, device)
 *                                  = their sum, the number of pairs; flags (F) one byte per face, or NULL: 1 iff the face is in some
 *                                  reported pair (zeroed first). ASYNC, capturable: no allocation, no synchronisation.
 *   ls_mesh_selfx_workspace_bytes  the workspace of ls_mesh_selfx_pairs for F faces and k pairs (256-byte aligned regions).
 *   ls_mesh_selfx_pairs            pairs (k, 2) int64 = the reported pairs (f, g), f < g, sorted lexicographically, from `counts` as
 *                                  ls_mesh_selfx_count filled them for the handle's current positions and k = its total. A pair past
 *                                  its face's count or past k is dropped, never written; counts of another mesh leave rows of
 *                                  zeros. k = 0 is a no-op. ASYNC.
 * LS_E_INVALID for a null required pointer or a negative size, LS_E_OVERFLOW when 3 F or 2 k reaches 2^31, LS_E_WORKSPACE for a
 * workspace below ls_mesh_selfx_workspace_bytes(F, k). The result depends on the mesh alone, not on the hierarchy: bitwise
 * reproducible. The calls only read the handle; none may overlap ls_mesh_distance_update or ls_mesh_distance_destroy of it.
 * --------------------------------------------------------------------------------------------- */
int ls_mesh_selfx_count(void* handle, int32_t* counts, int64_t* total, unsigned char* flags, void* stream);
int ls_mesh_selfx_workspace_bytes(int64_t F, int64_t k, size_t* bytes);
int ls_mesh_selfx_pairs(void* handle, const int32_t* counts, int64_t k, int64_t* pairs, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The level set S = iso of a scalar field on a regular grid as a triangle mesh, and the gradient of its vertices in the field
 * (largesteps/levelset.py). The rule is stated in csrc/isosurf.hip and DESIGN.md section 2.13 and restated in numpy by
 * tests/isosurf_statement.py, and the device answers with the same bits: marching tetrahedra on the Kuhn split. S (nx, ny, nz) fp32,
 * node (i, j, k) at origin + spacing * (i, j, k) with id (i ny + j) nz + k; every cube of 8 nodes is cut into the 6 tets c, c + e_a,
 * c + e_a + e_b, c + (1, 1, 1), one per permutation of the axes in lexicographic order, whose edges run along the 7 directions 100 010 001
 * 110 011 101 111 = slots 0..6 and belong to the node they start at. A node is low iff S < iso (a NaN is high); an edge is live iff
 * both ends are finite and exactly one is low; a cube with a non-finite corner emits nothing; a grid with a side of 1 has no cubes
 * and no vertices. One vertex per live edge, ordered by (node, slot) through an exclusive scan of the popcounts of the nodes' 7-bit
 * live masks: no sort, no atomics. With a the owner and b = a + d, in fp32: t = (iso - S[a]) / (S[b] - S[a]) clamped to [0, 1],
 * x = origin_x + spacing_x * ((float)i_a + t d_x). Faces are ordered by (cube, tet, triangle) through a second scan, by a 16-case
 * table, each with its normal from the low side to the high side.
 *   ls_iso_workspace_bytes  the workspace of the three calls below for an (nx, ny, nz) grid (256-byte aligned regions): the masks, the
 *                           counts and the two offset arrays.
 *   ls_iso_count            fills the workspace and totals (int64[2], device) = (the number of vertices, the number of faces).
 *                           ASYNC, capturable: no allocation, no synchronisation.
 *   ls_iso_fill             V (n, 3) fp32 the vertices, E (n) int64 = 8 node + slot, the grid edge of each vertex (or NULL), F (m, 3) int64
 *                           the faces, from the workspace as ls_iso_count filled it for the same S and iso. origin[3] and spacing[3]
 *                           are host arrays. A vertex past n or a face past m is dropped, never written. n = m = 0 is a no-op. ASYNC.
 *   ls_iso_backward         gS (nx, ny, nz) fp32, overwritten: the gradient of sum <gV, V> in S for gV (n, 3) fp32. Per live edge, in fp64
 *                           from the fp32 inputs: D = S[b] - S[a], t = (iso - S[a]) / D (no term unless 0 <= t <= 1), e = spacing * d,
 *                           term_a = (-(1 - t) / D) <gV, e>, term_b = (-t / D) <gV, e>. A node adds the term_a of its 7 slots in order, then
 *                           the term_b of the 7 edges owned by node - d in slot order, in fp64, rounded to fp32 once: no float
 *                           atomics, bitwise reproducible. A vertex past n adds nothing; n = 0 zeroes gS. ASYNC, capturable.
 * LS_E_INVALID for a null required pointer, a side below 1, a negative n or m, or a spacing that is not positive and finite;
 * LS_E_OVERFLOW when 8 x the nodes or 12 x the cubes reaches 2^31; LS_E_WORKSPACE for a workspace below ls_iso_workspace_bytes.
 * ls_iso_fill and ls_iso_backward only read the workspace; none may overlap an ls_iso_count on it.
 * --------------------------------------------------------------------------------------------- */
int ls_iso_workspace_bytes(int64_t nx, int64_t ny, int64_t nz, size_t* bytes);
int ls_iso_count(const float* S, int64_t nx, int64_t ny, int64_t nz, float iso, void* ws, size_t ws_bytes, int64_t* totals, int device,
                 void* stream);
int ls_iso_fill(const float* S, int64_t nx, int64_t ny, int64_t nz, float iso, const float* origin, const float* spacing, const void* ws,
                size_t ws_bytes, int64_t n, int64_t m, float* V, int64_t* E, int64_t* F, int device, void* stream);
int ls_iso_backward(const float* S, int64_t nx, int64_t ny, int64_t nz, float iso, const float* origin, const float* spacing,
                    const void* ws, size_t ws_bytes, int64_t n, const float* gV, float* gS, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Area-weighted points on a mesh surface and their gradient to the vertices (largesteps/sampling.py, and distance.chamfer_distance
 * built on it). The rule is stated in csrc/sample.hip and DESIGN.md section 2.9, restated in numpy by tests/sample_statement.py, and
 * the device answers with the same bits: fp64 areas from the fp32 corners quantised to 32 bits against the largest one, a 64-bit
 * integer prefix sum, Philox4x32-10 keyed by `seed` with the counter (sample index, stream_id, 0), and square-root barycentric weights.
 * A face without a finite positive area, or naming a vertex outside [0, V), is never drawn (no index is followed before it is checked).
 * verts (V, 3) fp32, faces (F, 3) int32 / int64 (idx_bytes 4 / 8). LS_E_INVALID for a null pointer, a negative size or another
 * idx_bytes; LS_E_OVERFLOW when n (within a workgroup of it), 3 F or offset + n reaches 2^31; LS_E_WORKSPACE for a workspace below
 * ls_sample_workspace_bytes(F, n). No entry point allocates or synchronises, none uses float atomics: bitwise reproducible. ASYNC.
 *   ls_sample_workspace_bytes   the workspace of either call below for F faces and n samples (256-byte aligned regions).
 *   ls_sample_surface           P (n, 3) fp32 the points, I (n) int64 their faces, W (n, 3) fp32 their barycentric weights, for the
 *                               samples offset .. offset + n - 1: the slice law -- samples [o, o + m) of any call are, bit for bit,
 *                               what the call with offset = o, n = m returns. When no face can be drawn (F = 0 included): P = NaN,
 *                               I = -1, W = 0, without an error.
 *   ls_sample_surface_backward  gV (V, 3) fp32, overwritten: gV[v] = sum_i W[i][k] gP[i] over the samples whose face I[i] has v at
 *                               corner k, from I and W as ls_sample_surface returned them (held fixed) and gP (n, 3) fp32. vptr (V + 1)
 *                               and corner_order (3 F) are the ranking of ls_corner_ranks over the same faces (corner_order: rank ->
 *                               corner, the inverse of its cpos), which carries the connectivity: `faces` itself is not read, and
 *                               the kernels index through the ranking without a range check. Samples of a face are added in
 *                               ascending i and a vertex's corners in rank order, in fp64, rounded to fp32 once. A sample whose I is
 *                               outside [0, F) adds nothing.
 * The 64-bit scan works in tiles of LS_SAMPLE_SCAN_TILE faces.
 * --------------------------------------------------------------------------------------------- */
#define LS_SAMPLE_SCAN_TILE 2048
int ls_sample_workspace_bytes(int64_t F, int64_t n, size_t* bytes);
int ls_sample_surface(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, int64_t n, uint64_t seed,
                      uint32_t stream_id, uint64_t offset, float* P, int64_t* I, float* W, void* ws, size_t ws_bytes, int device,
                      void* stream);
int ls_sample_surface_backward(const void* faces, int idx_bytes, int64_t F, int64_t V, int64_t n, const int64_t* I, const float* W,
                               const float* gP, const int32_t* vptr, const int32_t* corner_order, float* gV, void* ws, size_t ws_bytes,
                               int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * AdamUniform step (optimize.py:18-41) on n contiguous fp32 elements, two kernels, no host sync:
 *   g1 = b1 g1 + (1-b1) g ; g2 = b2 g2 + (1-b2) g^2 ; p -= lr * (g1/(1-b1^t)) / (1e-8 + max sqrt(g2/(1-b2^t)))
 * scratch: at least 4096 bytes of device memory owned by the caller. ASYNC.
 * --------------------------------------------------------------------------------------------- */
int ls_adam_uniform_step(float* param, const float* grad, float* g1, float* g2, int64_t n, float lr,
                         float beta1, float beta2, int step, void* scratch, int device, void* stream);
/* The same step with the step count ON THE DEVICE: d_step[0] = steps done so far (int32, zero before the first call; the call
 * increments it), d_step[1] = scratch. No argument changes from step to step, so the two launches can sit in a captured
 * graph (torch.cuda.graph around a whole optimisation step) and be replayed. ASYNC. */
int ls_adam_uniform_step_device(float* param, const float* grad, float* g1, float* g2, int64_t n, float lr, float beta1,
                                float beta2, int32_t* d_step, void* scratch, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable rasterizer (largesteps/render.py; the rules are stated in csrc/raster.hip and DESIGN.md section 2.7, restated in
 * numpy by tests/render_statement.py). pos (B, V, 4) fp32 clip-space positions, tri (F, 3) int32 whose indices lie in [0, V) (the
 * caller range-checks them: ls_corner_ranks does), resolution H x W up to 4096 each; rast (B, H, W, 4) fp32 = (u, v, z/w, id + 1), 0 for
 * background. vptr / corner_order: the corner ranking of ls_corner_ranks for tri (corner_order = rank -> corner, "order" above). No entry
 * point allocates or synchronises, none uses float atomics: outputs and gradients are bitwise reproducible. ASYNC.
 *   ls_raster_workspace_bytes       workspace of every entry point below for these sizes and C attribute / colour channels.
 *   ls_raster_forward               rast. Coverage: homogeneous edge functions in fp64 with a top-left rule, z/w in [-1, 1].
 *   ls_raster_pixel_order           order (B H W) = the pixels sorted stably by b F + face (background last), seg (B F + 1) = the first
 *                                   sorted position of each key: the order every backward sums in. Reads only rast's id channel.
 *   ls_raster_backward              grad_pos (B, V, 4) = d (sum grad_rast[..., 0:2] * (u, v)) / d pos; the z/w channel's gradient is
 *                                   dropped, grad_pos[..., 2] = 0. Overwritten.
 *   ls_raster_interpolate           out (B, H, W, C) = u a0 + v a1 + (1 - u - v) a2, 0 for background; attr (attr_batch, V, C) with
 *                                   attr_batch 1 (shared by every image) or B.
 *   ls_raster_interpolate_backward  grad_rast (B, H, W, 4) (channels 2, 3 zero) and grad_attr (attr_batch, V, C); either may be NULL.
 *   ls_raster_adjacency             adj (3 F): the face across edge (corner e, corner e + 1) of face f at adj[3 f + e], -1 when the
 *                                   edge has one face or more than two. Radix sort of the half-edges.
 *   ls_raster_antialias             out (B, H, W, C): the colour blended across silhouette edges between neighbouring pixels.
 *   ls_raster_antialias_backward    grad_color (B, H, W, C) and grad_pos (B, V, 4) (scaled by boost, [..., 2] = 0); either may be NULL.
 * --------------------------------------------------------------------------------------------- */
int ls_raster_workspace_bytes(int64_t B, int64_t F, int H, int W, int C, size_t* bytes);
int ls_raster_forward(const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W, float* rast, void* ws,
                      size_t ws_bytes, int device, void* stream);
int ls_raster_pixel_order(const float* rast, int64_t B, int64_t F, int H, int W, int32_t* order, int32_t* seg, void* ws, size_t ws_bytes,
                          int device, void* stream);
int ls_raster_backward(const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W, const float* grad_rast,
                       const int32_t* order, const int32_t* seg, const int32_t* vptr, const int32_t* corner_order, float* grad_pos,
                       void* ws, size_t ws_bytes, int device, void* stream);
int ls_raster_interpolate(const float* attr, int64_t attr_batch, int64_t V, int C, const float* rast, int64_t B, int H, int W,
                          const int32_t* tri, int64_t F, float* out, int device, void* stream);
int ls_raster_interpolate_backward(const float* attr, int64_t attr_batch, int64_t V, int C, const float* rast, int64_t B, int H, int W,
                                   const int32_t* tri, int64_t F, const float* grad_out, const int32_t* order, const int32_t* seg,
                                   const int32_t* vptr, const int32_t* corner_order, float* grad_attr, float* grad_rast, void* ws,
                                   size_t ws_bytes, int device, void* stream);
int ls_raster_adjacency_workspace_bytes(int64_t F, size_t* bytes);
int ls_raster_adjacency(const int32_t* tri, int64_t F, int32_t* adj, void* ws, size_t ws_bytes, int device, void* stream);
int ls_raster_antialias(const float* color, int C, const float* rast, const float* pos, int64_t B, int64_t V, int H, int W,
                        const int32_t* tri, int64_t F, const int32_t* adj, float* out, int device, void* stream);
int ls_raster_antialias_backward(const float* color, int C, const float* rast, const float* pos, int64_t B, int64_t V, int H, int W,
                                 const int32_t* tri, int64_t F, const int32_t* adj, const float* grad_out, float boost,
                                 const int32_t* order, const int32_t* seg, const int32_t* vptr, const int32_t* corner_order,
                                 float* grad_color, float* grad_pos, void* ws, size_t ws_bytes, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Range mode of the rasterizer (largesteps/render.py: rasterize(..., ranges=...); csrc/raster.hip). One pos
 * (V, 4) is shared; image b of B draws the faces tri[start_b : start_b + count_b]. ranges: a DEVICE int32 table (B, 3) = (start, count,
 * item_ptr), item_ptr the exclusive prefix sum of the counts, 0 <= start, 0 <= count, start + count <= F (the caller checks: the kernels
 * trust the table); ranges may overlap, be unsorted or empty. An item is a pair (b, f) with f in range b, numbered item_ptr[b] + f - start_b;
 * N = the sum of the counts. rast (B, H, W, 4) carries GLOBAL ids (face + 1). The slice law:
 *   image b is, bit for bit, what the instanced entry points give for pos as one batch and the faces tri[start_b : start_b + count_b],
 *   with start_b added to the id channel of covered pixels -- for the frame, the interpolation and the antialiasing -- and every gradient
 *   (grad_pos of ls_range_backward and of ls_range_antialias_backward, grad_attr, grad_color) is bit for bit the sum of the B slice calls'
 *   gradients, accumulated in ascending b starting from image 0's.
 * A pixel whose id is outside [start_b + 1, start_b + count_b] counts as background. Interpolation itself and its rast gradient are
 * ls_raster_interpolate / ls_raster_interpolate_backward with attr_batch 1 (ids are global, attr is shared). Limits: B >= 1; N, 3 N and
 * B H W fit int32; F < 2^24 (LS_E_INVALID / LS_E_OVERFLOW as above). No entry point allocates or synchronises, none uses float atomics. ASYNC.
 *   ls_range_workspace_bytes            workspace of the entry points below for B images, N items and C channels.
 *   ls_range_forward                    rast.
 *   ls_range_pixel_order                order (B H W) = the pixels sorted stably by item (background and foreign ids last), seg (N + 1).
 *   ls_range_backward                   grad_pos (V, 4) from grad_rast[..., 0:2]; grad_pos[..., 2] = 0. Overwritten.
 *   ls_range_interpolate_backward       grad_attr (V, C) from grad_out (B, H, W, C).
 *   ls_range_adjacency                  adj (3 N): the ITEM across edge e of item n at adj[3 n + e], -1 when the edge has one face or
 *                                       more than two WITHIN the image. Radix sort of the items' half-edges by (image, edge).
 *   ls_range_antialias                  out (B, H, W, C); silhouettes are those of each image's own faces.
 *   ls_range_antialias_backward         grad_color (B, H, W, C) and grad_pos (V, 4) (scaled by boost, [..., 2] = 0); either may be NULL.
 * --------------------------------------------------------------------------------------------- */
int ls_range_workspace_bytes(int64_t B, int64_t N, int H, int W, int C, size_t* bytes);
int ls_range_forward(const float* pos, int64_t V, const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N, int H, int W,
                     float* rast, void* ws, size_t ws_bytes, int device, void* stream);
int ls_range_pixel_order(const float* rast, const int32_t* ranges, int64_t B, int64_t N, int64_t F, int H, int W, int32_t* order,
                         int32_t* seg, void* ws, size_t ws_bytes, int device, void* stream);
int ls_range_backward(const float* pos, int64_t V, const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N, int H, int W,
                      const float* grad_rast, const int32_t* order, const int32_t* seg, const int32_t* vptr, const int32_t* corner_order,
                      float* grad_pos, void* ws, size_t ws_bytes, int device, void* stream);
int ls_range_interpolate_backward(const float* rast, const int32_t* ranges, int64_t B, int64_t N, int H, int W, int64_t V, int C,
                                  const float* grad_out, const int32_t* order, const int32_t* seg, const int32_t* vptr,
                                  const int32_t* corner_order, float* grad_attr, void* ws, size_t ws_bytes, int device, void* stream);
int ls_range_adjacency_workspace_bytes(int64_t N, size_t* bytes);
int ls_range_adjacency(const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N, int32_t* adj, void* ws, size_t ws_bytes,
                       int device, void* stream);
int ls_range_antialias(const float* color, int C, const float* rast, const float* pos, int64_t V, const int32_t* tri, int64_t F,
                       const int32_t* ranges, int64_t B, int64_t N, int H, int W, const int32_t* adj, float* out, int device, void* stream);
int ls_range_antialias_backward(const float* color, int C, const float* rast, const float* pos, int64_t V, const int32_t* tri, int64_t F,
                                const int32_t* ranges, int64_t B, int64_t N, int H, int W, const int32_t* adj, const float* grad_out,
                                float boost, const int32_t* order, const int32_t* seg, const int32_t* vptr, const int32_t* corner_order,
                                float* grad_color, float* grad_pos, void* ws, size_t ws_bytes, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth peeling of the rasterizer (largesteps/render.py: DepthPeeler; csrc/raster.hip): the layer behind a
 * previous one, in both modes. prev_rast (B, H, W, 4): the rast of the previous layer, as ls_raster_forward / ls_range_forward or an
 * earlier peel wrote it for the same pos, tri (ranges), H and W; it is only read, and must not be rast. The depth pass resolves a pixel
 * by the smallest key (order bits of fp32 z/w) << 32 | face, and rast keeps exactly that z/w and face + 1: the peel admits a covering
 * fragment only if its key is STRICTLY GREATER than the key of prev_rast at its pixel, and nothing where prev_rast is background or
 * holds an id that is not one of the image's. The law:
 *   layer l of a pixel (layer 0 = ls_raster_forward / ls_range_forward) is the l-th of the pixel's covering fragments in ascending
 *   (order bits of z/w, face) order, bit for bit as the forward pass would write that fragment; all zeros once they are used up.
 * Exact depth ties peel in face order; there is no epsilon. rast has the layout of the forward pass, so every other entry point
 * (pixel order, the backwards, interpolation, antialiasing) takes a layer as it takes a frame. Sizes, limits, error codes and the
 * workspace are those of ls_raster_forward (ls_raster_workspace_bytes) and ls_range_forward (ls_range_workspace_bytes); LS_E_INVALID
 * also when prev_rast is NULL or equals rast. Neither allocates or synchronises, neither uses float atomics. ASYNC.
 *   ls_peel_forward                 rast = the layer behind prev_rast, instanced mode.
 *   ls_peel_range_forward           the same in range mode (global ids, the slice law layer by layer).
 * --------------------------------------------------------------------------------------------- */
int ls_peel_forward(const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W, const float* prev_rast,
                    float* rast, void* ws, size_t ws_bytes, int device, void* stream);
int ls_peel_range_forward(const float* pos, int64_t V, const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N, int H,
                          int W, const float* prev_rast, float* rast, void* ws, size_t ws_bytes, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable 2D texture lookup (largesteps/render.py: texture; the rules are stated in csrc/texture.hip and DESIGN.md section 2.7,
 * restated in numpy by tests/texture_statement.py). tex (Bt, Ht, Wt, C) fp32 with Bt 1 (shared by every image) or B, 1 <= Ht, Wt <= 8192,
 * 1 <= C <= 32; uv (B, H, W, 2) fp32, 8-byte aligned; out (B, H, W, C). filter: LS_TEXTURE_NEAREST / _LINEAR; boundary: LS_TEXTURE_WRAP /
 * _CLAMP / _ZERO, applied per tap index. A non-finite uv gives output 0 and no gradient; every texel index is made range-safe before an
 * address is formed (saturating conversion, then integer remainder, clamp or range test). LS_E_INVALID for bad sizes or modes,
 * LS_E_OVERFLOW when B H W or Bt (Ht + 1) (Wt + 1) + 1 does not fit int32. No entry point allocates or synchronises, none uses float
 * atomics: outputs and gradients are bitwise reproducible. ASYNC.
 *   ls_texture_workspace_bytes   workspace of ls_texture_order for B H W pixels.
 *   ls_texture_forward           out.
 *   ls_texture_order             order (B H W) = the pixels sorted stably by their base tap (after the part of the boundary rule that does
 *                                not change which texels it touches; pixels without a gradient last), seg (Bt (Ht + 1) (Wt + 1) + 1) = the
 *                                first sorted position of each key: the order grad_tex sums in. Depends on uv, the texture's SHAPE and the
 *                                two modes only.
 *   ls_texture_backward          grad_tex (Bt, Ht, Wt, C) (summed over the images when Bt = 1) and grad_uv (B, H, W, 2) (zero for
 *                                LS_TEXTURE_NEAREST); either may be NULL, both are overwritten. order / seg: what ls_texture_order returned
 *                                for the same uv, shapes and modes (needed for grad_tex only; the kernels index pixels through them
 *                                without a range check).
 * --------------------------------------------------------------------------------------------- */
#define LS_TEXTURE_NEAREST 0
#define LS_TEXTURE_LINEAR 1
#define LS_TEXTURE_WRAP 0
#define LS_TEXTURE_CLAMP 1
#define LS_TEXTURE_ZERO 2
int ls_texture_workspace_bytes(int64_t B, int H, int W, size_t* bytes);
int ls_texture_forward(const float* tex, int64_t Bt, int Ht, int Wt, int C, const float* uv, int64_t B, int H, int W, int filter,
                       int boundary, float* out, int device, void* stream);
int ls_texture_order(const float* uv, int64_t B, int H, int W, int64_t Bt, int Ht, int Wt, int filter, int boundary, int32_t* order,
                     int32_t* seg, void* ws, size_t ws_bytes, int device, void* stream);
int ls_texture_backward(const float* tex, int64_t Bt, int Ht, int Wt, int C, const float* uv, int64_t B, int H, int W, int filter,
                        int boundary, const float* grad_out, const int32_t* order, const int32_t* seg, float* grad_tex, float* grad_uv,
                        int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mipmapped texture lookup and pixel differentials (largesteps/render.py: texture with the mipmap filter modes, texture_construct_mip,
 * pixel_differentials, interpolate(diff_attrs=...); the rules are stated in csrc/mip.hip and DESIGN.md section 2.7, restated in numpy
 * by tests/mip_statement.py). tex, uv, boundary as for ls_texture_*; Lmax in [0, 13] is the last level of the pyramid: every level
 * before it has sides that are 1 or even and is not 1 x 1 (LS_E_INVALID otherwise). pyr holds levels 1 .. Lmax packed one after the
 * other, level l as (Bt, H_l, W_l, C) with W_l = max(Wt >> l, 1); it may be NULL when Lmax = 0. uv_da (B, H, W, 4) fp32, 16-byte
 * aligned, and bias (B, H, W) fp32: either may be NULL, not both. mode: LS_MIP_NEAREST (linear-mipmap-nearest) / LS_MIP_LINEAR
 * (linear-mipmap-linear). LS_E_OVERFLOW when 2 B H W or the number of base positions of all levels does not fit int32. No entry point
 * allocates or synchronises, none uses float atomics: outputs and gradients are bitwise reproducible. ASYNC.
 *   ls_mip_workspace_bytes       workspace of ls_mip_order for B H W pixels.
 *   ls_mip_build                 pyr from tex: a texel is ((c00 + c10) + (c01 + c11)) * 0.25f of its children ((a + b) * 0.5f of two).
 *   ls_mip_fold                  the transpose of ls_mip_build, top down: every texel of level l (grad_tex for level 0) gains 0.25f
 *                                (0.5f) of its parent's gradient in grad_pyr. Call it after ls_mip_backward.
 *   ls_mip_pixel_differentials   out (B, H, W, 4) = (du/dX, du/dY, dv/dX, dv/dY) of the barycentrics in rast per pixel step, from the
 *                                clip-space pos (B, V, 4) and the int32 faces; 0 for background and degenerate faces.
 *   ls_mip_interpolate_da        out (B, H, W, 2 C) = [da_c/dX, da_c/dY] per channel from rast_db (the differentials above).
 *   ls_mip_forward               out (B, H, W, C).
 *   ls_mip_order                 order (2 B H W for LS_MIP_LINEAR, B H W for LS_MIP_NEAREST) = the items (pixel p at its lower level:
 *                                p; at its upper level: B H W + p) sorted stably by (level, base tap), items without a gradient last;
 *                                seg (K + 1), K = sum over the levels of Bt (H_l + 1) (W_l + 1). Depends on uv, uv_da, bias, the
 *                                SHAPES and the two modes only.
 *   ls_mip_backward              grad_tex (Bt, Ht, Wt, C) and grad_pyr (the layout of pyr): the gradient of every level BEFORE the fold;
 *                                grad_uv (B, H, W, 2); grad_lod (B, H, W) = d loss / d lod, which is the gradient of bias;
 *                                grad_uv_da (B, H, W, 4), which needs grad_lod. Any may be NULL; all given are overwritten.
 * --------------------------------------------------------------------------------------------- */
#define LS_MIP_NEAREST 0
#define LS_MIP_LINEAR 1
int ls_mip_workspace_bytes(int64_t B, int H, int W, size_t* bytes);
int ls_mip_build(const float* tex, int64_t Bt, int Ht, int Wt, int C, int Lmax, float* pyr, int device, void* stream);
int ls_mip_fold(float* grad_tex, int64_t Bt, int Ht, int Wt, int C, int Lmax, float* grad_pyr, int device, void* stream);
int ls_mip_pixel_differentials(const float* rast, const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W,
                               float* out, int device, void* stream);
int ls_mip_interpolate_da(const float* attr, int64_t attr_batch, int64_t V, int C, const float* rast, const float* rast_db, int64_t B,
                          int H, int W, const int32_t* tri, int64_t F, float* out, int device, void* stream);
int ls_mip_forward(const float* tex, const float* pyr, int64_t Bt, int Ht, int Wt, int C, int Lmax, const float* uv, const float* uv_da,
                   const float* bias, int64_t B, int H, int W, int mode, int boundary, float* out, int device, void* stream);
int ls_mip_order(const float* uv, const float* uv_da, const float* bias, int64_t B, int H, int W, int64_t Bt, int Ht, int Wt, int Lmax,
                 int mode, int boundary, int32_t* order, int32_t* seg, void* ws, size_t ws_bytes, int device, void* stream);
int ls_mip_backward(const float* tex, const float* pyr, int64_t Bt, int Ht, int Wt, int C, int Lmax, const float* uv, const float* uv_da,
                    const float* bias, int64_t B, int H, int W, int mode, int boundary, const float* grad_out, const int32_t* order,
                    const int32_t* seg, float* grad_tex, float* grad_pyr, float* grad_uv, float* grad_lod, float* grad_uv_da, int device,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable cube-map lookup (largesteps/render.py: texture with boundary_mode='cube'; the rules are stated in csrc/cube.hip and
 * DESIGN.md section 2.7, restated in numpy by tests/cube_statement.py). tex (Bt, 6, n, n, C) fp32 with Bt 1 (shared by every image) or B,
 * faces in the order +x, -x, +y, -y, +z, -z, 1 <= n <= 8192, 1 <= C <= 32; uv (B, H, W, 3) fp32: a direction that need not be
 * normalised; out (B, H, W, C). filter: LS_TEXTURE_NEAREST / _LINEAR. Linear taps that leave the face read the neighbouring face, a
 * tap beyond a corner is dropped and its weight shared by the other three. A direction with a non-finite component or with all
 * components zero gives output 0 and no gradient; every texel index is clamped into its range before an address is formed.
 * LS_E_INVALID for bad sizes, modes or null pointers, LS_E_OVERFLOW when 4 B H W or 6 Bt n^2 + 1 does not fit int32. No entry point
 * allocates or synchronises, none uses float atomics: outputs and gradients are bitwise reproducible. ASYNC.
 *   ls_cube_workspace_bytes      workspace of ls_cube_order for B H W pixels (16-byte aligned).
 *   ls_cube_forward              out.
 *   ls_cube_order                order (4 B H W for LS_TEXTURE_LINEAR: item 4 pixel + 2 dy + dx; B H W for LS_TEXTURE_NEAREST) = the
 *                                (pixel, tap) items sorted stably by their destination texel ((bt 6 + f) n + j) n + i, dropped taps and
 *                                pixels without a gradient last; seg (6 Bt n^2 + 1) = the first sorted position of each key: the order
 *                                grad_tex sums in. Depends on uv, the texture's SHAPE and the filter only.
 *   ls_cube_backward             grad_tex (Bt, 6, n, n, C) (summed over the images when Bt = 1) and grad_uv (B, H, W, 3) (zero for
 *                                LS_TEXTURE_NEAREST; the face choice is held fixed); either may be NULL, both are overwritten. order /
 *                                seg: what ls_cube_order returned for the same uv, shapes and filter (needed for grad_tex only; the
 *                                kernels index pixels through them without a range check).
 * --------------------------------------------------------------------------------------------- */
int ls_cube_workspace_bytes(int64_t B, int H, int W, size_t* bytes);
int ls_cube_forward(const float* tex, int64_t Bt, int n, int C, const float* uv, int64_t B, int H, int W, int filter, float* out,
                    int device, void* stream);
int ls_cube_order(const float* uv, int64_t B, int H, int W, int64_t Bt, int n, int filter, int32_t* order, int32_t* seg, void* ws,
                  size_t ws_bytes, int device, void* stream);
int ls_cube_backward(const float* tex, int64_t Bt, int n, int C, const float* uv, int64_t B, int H, int W, int filter,
                     const float* grad_out, const int32_t* order, const int32_t* seg, float* grad_tex, float* grad_uv, int device,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * One level of midpoint or Loop subdivision (libigl's upsample / loop) as a topology built once and a linear map S applied every step
 * (largesteps/subdivide.py). The rule is stated in csrc/subdiv.hip and DESIGN.md section 2.14 and restated in numpy by
 * tests/subdiv_statement.py, and the device answers with the same bits. Half-edge h = 3 f + e runs from F[f, e] to F[f, (e + 1) % 3];
 * the half-edges of one unordered vertex pair form an edge, owned by the one of lowest id; edges are numbered by ascending owner.
 * faces (F, 3) int32 / int64 (idx_bytes 4 / 8). The arrays of a topology, all device buffers of the caller:
 *   tri (3 F) int32       the faces narrowed
 *   he (3 F) int32        per half-edge: edge id << 2 | boundary << 1 | owner
 *   edges (E, 2) int32    the ends of edge e, the smaller id first: new vertex V + e sits on it   } both with room for 3 F rows:
 *   opp (E, 2) int32      the corners opposite the owner and opposite the other half-edge (or -1) } E is not known before the call
 *   valence (V) int32, bflag (V) uint8, bnbr (V, 2) int32   the number of edges at a vertex, whether it is a boundary vertex, and then
 *                         the far ends of its two boundary edges (else -1, -1)
 *   vptr (V + 1), order (3 F) int32   the corner ranking of ls_corner_ranks: the corners of v are order[vptr[v] .. vptr[v + 1])
 *   ls_subdiv_workspace_bytes  the workspace of ls_subdiv_topology (256-byte aligned regions).
 *   ls_subdiv_topology         fills the arrays above and fine_faces (4 F, 3) of the index type of `faces`; *h_E = E; *h_status = 0 or
 *                              the LS_SUBDIV_* flags of what is wrong with the mesh (the arrays then hold nothing of use, but nothing
 *                              was written or read out of bounds: a bad index is never followed). Radix sorts of the corners by vertex
 *                              and of the half-edges by (smaller end, larger end), an exclusive scan of the owner flags. SYNC (once).
 *   ls_subdiv_apply            out (V + E, C) fp32 = S X for X (V, C) fp32, 1 <= C <= 32, scheme LS_SUBDIV_MIDPOINT / _LOOP. Every row
 *                              is formed in fp64 from the fp32 inputs in the order the rule states and rounded once. ASYNC, capturable:
 *                              no allocation, no synchronisation.
 *   ls_subdiv_apply_backward   gX (V, C) fp32 = S^T g for g (V + E, C) fp32, overwritten: a gather per coarse vertex over the same walk,
 *                              fp64, rounded once, no float atomics, bitwise reproducible. ASYNC, capturable.
 * LS_E_INVALID for a null required pointer, a negative size, E > 3 F, C outside [1, 32], another idx_bytes or scheme; LS_E_OVERFLOW when
 * 12 F, V or V + E reaches 2^31; LS_E_WORKSPACE for a workspace below ls_subdiv_workspace_bytes. The apply calls follow the arrays
 * without a range check: they must come from an ls_subdiv_topology that returned status 0 for the same F and V.
 * --------------------------------------------------------------------------------------------- */
#define LS_SUBDIV_MIDPOINT 0
#define LS_SUBDIV_LOOP 1
#define LS_SUBDIV_BAD_INDEX 1          /* a face index outside [0, V) */
#define LS_SUBDIV_REPEATED_VERTEX 2    /* a face names a vertex twice */
#define LS_SUBDIV_NONMANIFOLD_EDGE 4   /* an edge with more than two half-edges */
#define LS_SUBDIV_NONMANIFOLD_VERTEX 8 /* a vertex with a number of boundary edges other than 0 or 2 */
int ls_subdiv_workspace_bytes(int64_t F, int64_t V, size_t* bytes);
int ls_subdiv_topology(const void* faces, int idx_bytes, int64_t F, int64_t V, int32_t* tri, int32_t* he, int32_t* edges, int32_t* opp,
                       int32_t* valence, unsigned char* bflag, int32_t* bnbr, int32_t* vptr, int32_t* order, void* fine_faces,
                       int64_t* h_E, int* h_status, void* ws, size_t ws_bytes, int device, void* stream);
int ls_subdiv_apply(const float* X, int64_t F, int64_t V, int64_t E, int C, int scheme, const int32_t* tri, const int32_t* he,
                    const int32_t* edges, const int32_t* opp, const int32_t* valence, const unsigned char* bflag, const int32_t* bnbr,
                    const int32_t* vptr, const int32_t* order, float* out, int device, void* stream);
int ls_subdiv_apply_backward(const float* g, int64_t F, int64_t V, int64_t E, int C, int scheme, const int32_t* tri, const int32_t* he,
                             const int32_t* edges, const int32_t* opp, const int32_t* valence, const unsigned char* bflag,
                             const int32_t* bnbr, const int32_t* vptr, const int32_t* order, float* gX, int device, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh topology (libigl's vertex_components / facet_components / boundary_loop / remove_unreferenced, largesteps/topology.py): the
 * components of a triangle mesh, its edges with their faces and flags, its boundary loops, the area and signed volume of every facet
 * component, and the compaction that keeps some of them. The rule is stated in csrc/topology.hip and DESIGN.md section 2.15 and
 * restated in numpy by tests/topology_statement.py; the device returns the statement's arrays, the fp64 measures bit for bit. Half-edges
 * and edges are those of ls_subdiv_*: edge e of ls_topo_build is edge e of ls_subdiv_topology. Components come from hooking the larger
 * root under the smaller with integer atomicMin and one compression: the root of a component is its lowest id whatever the
 * interleaving, so the labels are deterministic. faces (F, 3) int32 / int64 (idx_bytes 4 / 8). The arrays, all device buffers of the caller:
 *   tri (3 F) int32             the faces narrowed
 *   vcomp (V), fcomp (F) int32  the vertex component of a vertex (numbered by ascending lowest vertex id; a vertex in no face is its own)
 *                               and the facet component of a face (faces that share an EDGE, numbered by ascending lowest face id)
 *   edges (E, 2) int32          the ends of edge e, the smaller id first                                      } with room for 3 F rows:
 *   edge_faces (E, 2) int32     the faces of the edge's two lowest half-edges, the second -1 on a boundary    } E is not known before
 *   eflag (E) uint8             LS_TOPO_EDGE_BOUNDARY / _NONMANIFOLD / _MISORIENTED                           } the call
 *   corder (3 F) int32          the corners sorted stably by vertex
 *   forder (F), fseg (F + 2) int32   the faces grouped by facet component: those of k are forder[fseg[k] .. fseg[k + 1]), ascending
 *   loops (V), loop_ptr (V + 1) int32   the B boundary vertices loop after loop: loop l is loops[loop_ptr[l] .. loop_ptr[l + 1]), from
 *                               its lowest vertex along the boundary half-edges, the loops by ascending lowest vertex
 *   ls_topo_workspace_bytes       the workspace of ls_topo_build (256-byte aligned regions).
 *   ls_topo_build                 fills the arrays above. h_sizes[LS_TOPO_SIZES] = E, vertex components, facet components, B, loops,
 *                                 boundary edges, non-manifold edges, misoriented edges; *h_status = 0 or LS_TOPO_* flags. With
 *                                 LS_TOPO_BAD_INDEX or _REPEATED_VERTEX the arrays hold nothing of use; with LS_TOPO_BAD_BOUNDARY (a
 *                                 boundary vertex without exactly one boundary half-edge leaving and one entering) only loops and
 *                                 loop_ptr do not. Nothing is read or written out of bounds in either case: a bad index is never
 *                                 followed. No host loop over device results: SYNC (once, at the end).
 *   ls_topo_counts                counts (K, 6) int64, zeroed first: per facet component its faces, distinct vertices, edges, boundary,
 *                                 non-manifold and misoriented edges. Integer atomic adds, one per wave where its lanes share a
 *                                 component. ASYNC, capturable.
 *   ls_topo_measures              out (K, 2) fp64 = area and signed volume of every facet component from verts (V, 3) fp32; terms
 *                                 (F, 2) fp64 is the caller's scratch for the per-face terms. The sums run in the one order of the
 *                                 segmented sum of csrc/groupby.h over a component's faces in ascending id: no float atomics, bitwise
 *                                 reproducible. ASYNC, capturable: no allocation, no synchronisation.
 *   ls_topo_keep_workspace_bytes  the workspace of ls_topo_keep.
 *   ls_topo_keep                  mask (K) uint8 over the facet components. faces_out (cap_faces, 3), I (V) and J (cap_vertices) of
 *                                 idx_bytes: the kept faces in their order renumbered through I, I[v] = the new id of v or -1,
 *                                 J = the kept vertices in ascending old id; sizes[2] (device, int64) = the kept faces and vertices.
 *                                 Rows past cap_faces / cap_vertices are dropped, never written. ASYNC, capturable.
 * LS_E_INVALID for a null required pointer, a negative size, E > 3 F, K > F or another idx_bytes; LS_E_OVERFLOW when 3 F or V reaches
 * 2^31; LS_E_WORKSPACE for a workspace below the size function's answer. counts, measures and keep follow the arrays without a range
 * check: they must come from an ls_topo_build that returned no LS_TOPO_BAD_INDEX / _REPEATED_VERTEX for the same F and V.
 * --------------------------------------------------------------------------------------------- */
#define LS_TOPO_BAD_INDEX 1            /* a face index outside [0, V) */
#define LS_TOPO_REPEATED_VERTEX 2      /* a face names a vertex twice */
#define LS_TOPO_BAD_BOUNDARY 4         /* the boundary is not a set of oriented cycles */
#define LS_TOPO_EDGE_BOUNDARY 1        /* an edge of one half-edge */
#define LS_TOPO_EDGE_NONMANIFOLD 2     /* an edge of more than two half-edges */
#define LS_TOPO_EDGE_MISORIENTED 4     /* an edge of exactly two half-edges that run the same way */
#define LS_TOPO_SIZES 8
int ls_topo_workspace_bytes(int64_t F, int64_t V, size_t* bytes);
int ls_topo_build(const void* faces, int idx_bytes, int64_t F, int64_t V, int32_t* tri, int32_t* vcomp, int32_t* fcomp, int32_t* edges,
                  int32_t* edge_faces, unsigned char* eflag, int32_t* corder, int32_t* forder, int32_t* fseg, int32_t* loops,
                  int32_t* loop_ptr, int64_t* h_sizes, int* h_status, void* ws, size_t ws_bytes, int device, void* stream);
int ls_topo_counts(const int32_t* tri, const int32_t* fcomp, const int32_t* edge_faces, const unsigned char* eflag, const int32_t* corder,
                   int64_t F, int64_t E, int64_t K, int64_t* counts, int device, void* stream);
int ls_topo_measures(const float* verts, const int32_t* tri, const int32_t* forder, const int32_t* fseg, int64_t F, int64_t V, int64_t K,
                     double* terms, double* out, int device, void* stream);
int ls_topo_keep_workspace_bytes(int64_t F, int64_t V, size_t* bytes);
int ls_topo_keep(const int32_t* tri, const int32_t* fcomp, const unsigned char* mask, int64_t F, int64_t V, int64_t K, int idx_bytes,
                 int64_t cap_faces, int64_t cap_vertices, void* faces_out, void* I, void* J, int64_t* sizes, void* ws, size_t ws_bytes,
                 int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LARGESTEPS_HIP_H */
