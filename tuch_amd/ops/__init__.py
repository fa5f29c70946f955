"""torch-facing wrappers over the C ABI: device tensors in, device tensors out.

Everything here runs the hand-written HIP kernels of libtuch_amd.so; there is no
eager/CPU fallback.  Index outputs are int64 like the reference's torch ops.

One module per kernel family, each named after the csrc files it binds, imported in this order (a module imports only
from the ones above it):

    _base           streams, workspaces, tickets, the deterministic switch, the hand-over of unit gradients
    args            the rules for caller arguments (``ops.args.rho_of`` ...): the one module callers read by name
    dense           pairwise distances, solid angles, winding numbers, the masked nearest vertex
    selfcontact     self-contact detection
    normals_render  vertex normals, the mesh renderer, the contact colouring
    terms           the contact terms
    objectives      the SMPLify-DC stage-1 and stage-2 objectives
    mesh_fit        the fit to meshes in correspondence, the transfer table
    closest_point   closest point on the posed surface, the point-to-surface term
    model           ContactModel and its table builders
    point_cloud     PointCloud and the model-to-scan term
    hd              the HD branch
    image_crop      the regressor's input crops

This file only re-exports their public names: callers say ``ops.scan_fit(...)``, whichever module owns it.
"""
from ..backward_pass import backward_scalar          # (the fitting loops and the bench call ops.backward_scalar)
from . import args
from ._base import (as_u8, cached_derived, deterministic, deterministic_mode, off_default_stream, set_deterministic)
from .args import MAX_NEIGHBOURS, SCAN_RHO
from .dense import (batch_pairwise_dist, gather_triangles, pack_geomask, solid_angles, v2v_min_masked, winding_numbers)
from .selfcontact import MAX_CONTACT_REGIONS, self_contact, vertex_region_table
from .normals_render import (MAX_RENDER_VIEWS, VertexNormalTable, contact_vertex_colors, render_mesh, vertex_face_table,
                             vertex_normal_table, vertex_normals)
from .terms import MODE_SMPLIFY, MODE_TRAIN, contact_terms, contact_terms_mean, contact_terms_ragged, valid_mean
from .objectives import smplify_objective, smplify_small_terms, smplify_stage1_objective, smplify_stage2_tail
from .mesh_fit import FitWeights, TransferTable, fit_weights, mesh_transfer, transfer_table, vertex_fit
from .closest_point import ClosestPoint, scan_fit
from .model import ContactModel, cluster_tree, near_encode_host, region_tables, segment_faces
from .point_cloud import CloudGrid, KNearest, NearestPoint, PointCloud, PointNormals, cloud_fit, set_cloud_canary
from .hd import HDModel, hd_points
from .image_crop import (CROP_FRAC_BITS, CROP_MAX_K, CROP_MAX_RES, CROP_RECORD, IMAGE_TABLE, DeviceCropRecords,
                         check_crop_records, crop_batch, crop_box, crop_records, pack_images, upload_crop_records)
