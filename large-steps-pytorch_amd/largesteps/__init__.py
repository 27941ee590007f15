"""
largesteps -- MI355X-native implementation of the Laplacian parameterization hot path of
"Large Steps in Inverse Rendering of Geometry" (reference package: rgl-epfl/large-steps-pytorch,
largesteps/ 0.2.2). Same modules, symbols and call forms as the reference:

    from largesteps.geometry import compute_matrix, laplacian_uniform, laplacian_cot
    from largesteps.parameterize import to_differential, from_differential
    from largesteps.solvers import CholeskySolver, ConjugateGradientSolver, solve
    from largesteps.optimize import AdamUniform
    from largesteps.normals import compute_face_normals, compute_vertex_normals     (reference: scripts/geometry.py)
    import largesteps.render as dr       (nvdiffrast.torch's rasterize / interpolate / antialias; NVDRenderer: scripts/render.py)
    from largesteps.distance import hausdorff, point_mesh_squared_distance   (igl's: the figures' error column)
    from largesteps.sampling import sample_surface; from largesteps.distance import chamfer_distance   (mesh-to-mesh measures)
    from largesteps.raycast import RayMesh, ray_mesh_intersect, ambient_occlusion   (igl's ray queries, on the distance handle's LBVH)
    from largesteps.subdivide import Subdivision, loop, upsample   (igl's loop / upsample as a linear map applied every step)
    from largesteps.topology import MeshTopology, facet_components, boundary_loops, keep_largest_component   (igl's components and loops)

Device work is done by hand-written HIP kernels for gfx950 in lib/liblargesteps_hip.so (C ABI in
include/largesteps_hip.h); there is no CPU or stock-PyTorch fallback.
"""

__version__ = "0.2.2+mi355x.2"
__author__ = "largesteps-mi355x contributors (API after Baptiste Nicolet's largesteps)"
