"""thr3ed_atom_amd -- MI355X-native ReLU-Fields volume rendering hot path.

Host-side mirror of the reference's render interface (Rays / RenderOut / VoxelGrid /
SHVoxGridRenderConfig / render_sh_voxel_grid / VolumetricModel) over hand-written gfx950 HIP kernels
reached through the C ABI in include/relu_field.h.  Importing the package does not need a GPU; calling
the render path does, and it raises instead of falling back when the HIP library or a GPU is missing.
"""
from .camera import (  # noqa: F401
    CameraBounds,
    CameraIntrinsics,
    CameraPose,
    compute_expected_density_scale_for_relu_field_grid,
    compute_thre3d_grid_sizes,
    get_thre360_animation_poses,
    get_thre360_spiral_animation_poses,
    mse2psnr,
    perturb_pose,
    pose_spherical,
    scale_camera_intrinsics,
    so3_exp,
)
from .render_interface import (  # noqa: F401
    Rays,
    RenderOut,
    collate_rays,
    collate_rendered_output,
    flatten_rays,
    reshape_rendered_output,
)
from .voxels import (  # noqa: F401
    AxisAlignedBoundingBox,
    VoxelGrid,
    VoxelGridLocation,
    VoxelSize,
    create_voxel_grid_from_saved_info_dict,
    scale_voxel_grid_with_required_output_size,
)
from .renderers import SHVoxGridRenderConfig, density2occupancy_pb, render_sh_voxel_grid, render_sh_voxel_grid_frame, render_sh_voxel_grid_pair  # noqa: F401
from .volumetric_model import VolumetricModel, cast_rays, create_volumetric_model_from_saved_model  # noqa: F401
from .composable import (  # noqa: F401  (the path at the granularity of the reference's plug-in points)
    SampledPointsOnRays,
    accumulate_radiance_density_on_rays,
    process_points_with_sh_voxel_grid,
    render,
    sample_aabb_bound_uniform_points_on_rays,
    sample_uniform_points_on_rays,
)
from .mesh import Mesh, extract_mesh, write_ply  # noqa: F401
from .mesh_simplify import MeshSimplifyStats, simplify_mesh  # noqa: F401
from .texture import TextureBake, ViewBake, bake_texture, bake_texture_from_field_views, bake_texture_from_views, write_obj  # noqa: F401
from .mesh_raster import MeshRender, evaluate_mesh_against_field, read_obj, render_mesh  # noqa: F401
from .texture_fit import MeshTextureSampler, TextureFit, fit_texture, fit_texture_to_field_views  # noqa: F401
from .mesh_fit import MeshFit, MeshGeometryRenderer, fit_mesh_to_field_views, fit_mesh_to_views  # noqa: F401
from .fusion import FusedVolume, fuse_depth_views, fuse_field_views  # noqa: F401
from .mesh_distance import ClosestPoints, DirectedDistance, MeshDistance, MeshDistanceGrid, ThresholdScore, closest_points_on_mesh, mesh_distance, sample_mesh_surface  # noqa: F401
from .mesh_distance_grad import MeshChamferLoss, fit_mesh_to_mesh, mesh_surface_points, point_mesh_distance  # noqa: F401
from .mesh_sign import (MeshSDF, MeshSignGrid, MeshTopology, SignedClosestPoints, SignedDirected, SignedMeshDistance, mesh_contains, mesh_signed_distance,  # noqa: F401
                        mesh_to_sdf, mesh_topology, point_mesh_signed_distance, signed_mesh_distance)
from .ops import distortion_loss, render_geometry, total_variation  # noqa: F401
from .metrics import ssim  # noqa: F401
from .trainers import evaluate_sh_vox_grid_vol_mod_with_posed_images  # noqa: F401
from .geometry import back_project_points, normal_map_image, write_point_cloud_ply  # noqa: F401
from .pose_refinement import pose_error, refine_camera_pose  # noqa: F401
from .pruning import PruneStats, node_max_weights, prune_voxel_grid  # noqa: F401
from .resampling import TightenStats, content_bounds, crop_voxel_grid, resample_voxel_grid, tighten_voxel_grid  # noqa: F401
from .components import ComponentStats, Components, label_components, remove_small_components  # noqa: F401
from .compression import CompressedField, compress_voxel_grid, partition_by_shares, vq_assign, vq_kmeans, vq_update_centroids  # noqa: F401

__version__ = "0.1.0"
