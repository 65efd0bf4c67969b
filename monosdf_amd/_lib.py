"""ctypes binding of libmonosdf_hip.so (C ABI declared in include/monosdf_hip.h and the additive headers beside it).

The product path has no CPU or eager-PyTorch fallback: if the shared library is
missing or a kernel launch fails, this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MONOSDF_HIP_LIB: another build of the same library (kernel tuning experiments), never a different backend
LIB_PATH = os.environ.get('MONOSDF_HIP_LIB') or os.path.join(_HERE, 'libmonosdf_hip.so')

MAX_LAYERS = 10
MAX_TILES = 17


class _NoDict(type(C.Structure)):
    def __new__(mcs, name, bases, namespace):
        namespace.setdefault('__slots__', ())
        return super().__new__(mcs, name, bases, namespace)


class Struct(C.Structure, metaclass=_NoDict):
    """Base of every mirror of a C struct.  Its instances have no __dict__, so assigning to a name that is no field
    raises AttributeError (a plain ctypes.Structure would accept it and leave the field it was meant for zero)."""

    def __reduce__(self):
        # ctypes' own __reduce__ reads __dict__; as there, a struct that holds addresses is not copied or pickled
        if any(ctype is C.c_void_p for _, ctype in self._fields_):
            raise ValueError('monosdf_amd: %s holds addresses and cannot be copied or pickled' % type(self).__name__)
        return type(self).from_buffer_copy, (bytes(self),)


class Layer(Struct):
    _fields_ = [(n, C.c_int32) for n in
                ('kt', 'ot', 'wf_off', 'wb_off', 'bias_off', 'skip_tile', 'hpre', 'qpre', 'abpre',
                 'ktp', 'otp', 'pad_')]


class Plan(Struct):
    _fields_ = [(n, C.c_int32) for n in
                ('n_layers', 'e_tiles', 'aux_tiles', 'n_freqs', 'sdf_slot', 'feat_tiles', 'hsum',
                 'qsum', 'absum', 'wsdf_off', 'mode', 'out_act', 'precision', 'out_rows')] + [('layer', Layer * MAX_LAYERS)]


class PackRule(Struct):
    _fields_ = [('w_off', C.c_int32), ('b_off', C.c_int32), ('rows', C.c_int32), ('cols', C.c_int32),
                ('rowmap_off', C.c_int32), ('colmap_off', C.c_int32), ('scale', C.c_float),
                ('pad_', C.c_int32)]


class WgradItem(Struct):
    _fields_ = [('x', C.c_int64), ('y', C.c_int64), ('v', C.c_int64),
                ('part_off', C.c_int64), ('colsum_off', C.c_int64), ('vrow_off', C.c_int64),
                ('x_ld', C.c_int32), ('y_ld', C.c_int32), ('wx', C.c_int32), ('wy', C.c_int32),
                ('n_splits', C.c_int32), ('bufs', C.c_int32)]


class ReduceRule(Struct):
    _fields_ = [('part_off', C.c_int64), ('dst_off', C.c_int64), ('n_blocks', C.c_int32),
                ('wx', C.c_int32), ('wy', C.c_int32), ('rowmap_off', C.c_int32),
                ('colmap_off', C.c_int32), ('dst_ld', C.c_int32), ('fixed_row', C.c_int32),
                ('scale', C.c_float)]


_P = C.c_void_p


class FgArgs(Struct):
    _fields_ = [('wpack', _P), ('bpack', _P), ('x', _P), ('aux', _P),
                ('P', C.c_int32), ('P_pad', C.c_int32), ('n_clamp', C.c_int32), ('n_feat', C.c_int32),
                ('clamp_radius', C.c_float), ('sphere_scale', C.c_float),
                ('sdf', _P), ('feat', _P), ('nrm', _P), ('r_aux', _P), ('clamped', _P),
                ('H', _P), ('PM', _P), ('IN0', _P), ('save', C.c_int32), ('aux_C', C.c_int32), ('aux_LC', C.c_int32),
                ('aux_dx_scale', C.c_float), ('dy_dx', _P),
                ('row_map', _P), ('smp_flags', _P), ('h_saved', _P), ('n_reuse', C.c_int32), ('stage_pad', C.c_int32), ('h_stage', _P),
                ('wg_first', C.c_int32)]


class BwArgs(Struct):
    _fields_ = [('wpack', _P), ('bpack', _P), ('x', _P),
                ('P', C.c_int32), ('P_pad', C.c_int32), ('n_feat', C.c_int32), ('n_split', C.c_int32),
                ('g_sdf', _P), ('g_feat', _P), ('g_nrm', _P), ('g_raux', _P), ('clamped', _P),
                ('H', _P), ('PM', _P), ('QB', _P), ('T', _P), ('AB', _P), ('GSDF', _P), ('QLAST', _P),
                ('g_aux', _P), ('g_sdf_b', _P), ('g_nrm_b', _P), ('aux_C', C.c_int32), ('aux_LC', C.c_int32),
                ('dy_dx', _P), ('gg_out', _P), ('aux_dx_scale', C.c_float), ('pad_', C.c_int32),
                ('row_map', _P)]


class ColorFwdArgs(Struct):
    _fields_ = [('wpack', _P), ('bpack', _P), ('x', _P), ('dirs', _P), ('nrm', _P), ('feat', _P),
                ('code', _P), ('P', C.c_int32), ('P_pad', C.c_int32), ('spr', C.c_int32),
                ('save', C.c_int32), ('rgb', _P), ('H', _P), ('MISC', _P)]


class ColorBwdArgs(Struct):
    _fields_ = [('wpack', _P), ('bpack', _P), ('rgb', _P), ('g_rgb', _P),
                ('P', C.c_int32), ('P_pad', C.c_int32), ('H', _P), ('AB', _P), ('g_feat', _P),
                ('g_misc', _P), ('g_nrm', _P)]


class CompositeArgs(Struct):
    _fields_ = [('z', _P), ('sdf', _P), ('rgb', _P), ('nrm', _P), ('beta', _P), ('depth_scale', _P),
                ('N', C.c_int32), ('S', C.c_int32), ('white_bkgd', C.c_int32),
                ('bg0', C.c_float), ('bg1', C.c_float), ('bg2', C.c_float),
                ('weights', _P), ('rgb_values', _P), ('depth_values', _P), ('normal_map', _P),
                ('wsum', _P), ('pose', _P), ('pose_stride', C.c_int32), ('depth_scale_stride', C.c_int32),
                ('depth_vals', _P)]


class CompositeBwdArgs(Struct):
    _fields_ = [('z', _P), ('sdf', _P), ('rgb', _P), ('nrm', _P), ('beta', _P), ('depth_scale', _P),
                ('weights', _P), ('wsum', _P), ('depth_values', _P), ('g_rgb_values', _P),
                ('g_depth', _P), ('g_normal', _P), ('g_weights', _P),
                ('N', C.c_int32), ('S', C.c_int32), ('white_bkgd', C.c_int32),
                ('bg0', C.c_float), ('bg1', C.c_float), ('bg2', C.c_float),
                ('g_sdf', _P), ('g_rgb', _P), ('g_nrm', _P), ('g_beta_part', _P),
                ('pose', _P), ('pose_stride', C.c_int32), ('depth_scale_stride', C.c_int32)]


class WnLayer(Struct):
    _fields_ = [('v', _P), ('g', _P), ('b', _P), ('rows', C.c_int32), ('cols', C.c_int32),
                ('w_off', C.c_int32), ('b_off', C.c_int32), ('row_off', C.c_int32), ('has_g', C.c_int32)]


class ProbeLossArgs(Struct):
    _fields_ = [('rgb', _P), ('nrm', _P), ('depth', _P), ('g1', _P), ('g2', _P), ('N', C.c_int32), ('M', C.c_int32),
                ('w_normal', C.c_float), ('w_depth', C.c_float), ('w_eik', C.c_float), ('w_smooth', C.c_float),
                ('g_rgb', _P), ('g_nrm', _P), ('g_depth', _P), ('g_g1', _P), ('g_g2', _P), ('partial', _P)]


class MonoSdfLossArgs(Struct):
    _fields_ = [(n, _P) for n in ('rgb', 'depth', 'normal', 'sdf', 'grad_theta', 'grad_nei', 'rgb_gt', 'depth_gt',
                                  'normal_gt', 'mask_gt')] + \
               [(n, C.c_int32) for n in ('N', 'S', 'E', 'gamma', 'scale_invariant')] + \
               [(n, C.c_float) for n in ('w_eik', 'w_smooth', 'w_depth', 'w_nl1', 'w_ncos')] + \
               [(n, _P) for n in ('mask', 'out', 'g_rgb', 'g_depth', 'g_normal', 'g_theta', 'g_nei')]


class SamplerArgs(Struct):
    _fields_ = [('ray_o', _P), ('ray_d', _P), ('N', C.c_int32), ('M', C.c_int32), ('m_max', C.c_int32),
                ('n_eval', C.c_int32), ('n_final', C.c_int32), ('n_extra', C.c_int32),
                ('round_idx', C.c_int32), ('max_rounds', C.c_int32), ('training', C.c_int32),
                ('beta_iters', C.c_int32), ('near', C.c_float), ('far', C.c_float), ('bound', C.c_float),
                ('eps', C.c_float), ('add_tiny', C.c_float), ('lemma', C.c_float),
                ('beta0', _P), ('z', _P), ('sdf', _P), ('new_z', _P), ('new_sdf', _P), ('new_pos', _P),
                ('pts', _P), ('beta', _P), ('flags', _P), ('jitter', _P), ('u_final', _P), ('final_z', _P),
                ('extra_idx', _P), ('eik_idx', _P), ('z_out', _P), ('z_eik', _P), ('pts_out', _P),
                ('eik_uniform', _P), ('nei_rand', _P), ('far_out', _P), ('rounds_out', _P),
                ('dbg_dstar', _P), ('dbg_err0', _P), ('dbg_cdf', _P), ('eik_u', _P), ('eik_unit', C.c_int32),
                ('pad_', C.c_int32), ('row_map', _P), ('h_saved', _P)]


_ERR = {1: 'invalid argument', 2: 'kernel launch failed', 3: 'unsupported configuration'}

ABI_VERSION = 8
VERSIONED_HEADER = 'monosdf_hip.h'

# The whole C ABI: header under include/ -> {entry: argtypes}; the return type is int, int64_t for a name that ends in
# _bytes.  The first header is the versioned surface (ABI_VERSION, exported_symbols()); the others are additive, one
# per feature, and leave that version alone.  load() binds what is here and nothing else, so an entry point of a new
# header is one more key (tests/test_abi_cpu.py holds every header under include/ against its key).
_ABI = {VERSIONED_HEADER: {
    'msdf_abi_version': [],
    'msdf_hash_encode_forward': [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_float, C.c_uint32, C.c_int, _P, _P],
    'msdf_hash_encode_backward': [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_float, C.c_uint32, C.c_int, _P, _P, _P],
    'msdf_hash_encode_second_backward': [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_float, C.c_uint32, C.c_int, _P, _P, _P, _P, _P],
    'msdf_hash_scatter_workspace_bytes': [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64],
    'msdf_hash_encode_backward_ws': [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_float, C.c_uint32, C.c_int, _P, _P, C.c_uint64, _P, C.c_uint64, _P],
    'msdf_hash_encode_second_backward_ws': [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_float, C.c_uint32, C.c_int, _P, _P, _P, _P, C.c_uint64, _P,
                                            C.c_uint64, _P],
    'msdf_hash_encode_backward_fused': [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_float, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, _P],
    'msdf_hash_encode_backward_fused_out': [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_float, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, _P],
    'msdf_hash_node_forward': [_P, C.c_double, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                               C.c_float, C.c_uint32, _P, _P],
    'msdf_hash_node_input_gradient': [_P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _P, _P],
    'msdf_hash_node_second_grad': [_P, _P, C.c_uint32, C.c_float, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_uint32, _P],
    'msdf_hash_transpose': [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P],
    'msdf_hash_node_scatter': [_P, _P, C.c_uint32, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                               C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, _P],
    'msdf_weightnorm_forward': [_P, _P, C.c_int, _P, _P, _P, _P],
    'msdf_weightnorm_backward': [_P, _P, C.c_int, _P, _P, _P, _P, _P],
    'msdf_pack_weights': [C.POINTER(Plan), _P, _P, _P, _P, _P, _P, _P],
    'msdf_sdf_forward': [C.POINTER(Plan), _P, _P, _P, _P, C.c_int, C.c_float, C.c_float, _P, _P],
    'msdf_sdf_forward_if': [C.POINTER(Plan), _P, _P, _P, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P],
    'msdf_sdf_forward_lm': [C.POINTER(Plan), _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, _P],
    'msdf_sdf_forward_save': [C.POINTER(Plan), _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P,
                              _P, C.c_int, _P, C.c_int, C.c_int, _P, _P],
    'msdf_sdf_fwd_grad': [C.POINTER(Plan), C.POINTER(FgArgs), _P],
    'msdf_sdf_backward': [C.POINTER(Plan), C.POINTER(BwArgs), _P],
    'msdf_color_forward': [C.POINTER(Plan), C.POINTER(ColorFwdArgs), _P],
    'msdf_color_backward': [C.POINTER(Plan), C.POINTER(ColorBwdArgs), _P],
    'msdf_wgrad': [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P],
    'msdf_camera_rays': [_P, _P, _P, C.c_int, _P, _P, _P, _P],
    'msdf_pixel_rays': [_P, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P],
    'msdf_monosdf_loss': [C.POINTER(MonoSdfLossArgs), _P],
    'msdf_reduce': [_P, C.c_int, _P, _P, _P, _P],
    'msdf_composite_forward': [C.POINTER(CompositeArgs), _P],
    'msdf_composite_backward': [C.POINTER(CompositeBwdArgs), _P],
    'msdf_beta_eff': [_P, C.c_float, _P, _P],
    'msdf_beta_grad': [_P, _P, C.c_int, _P, _P],
    'msdf_probe_loss': [C.POINTER(ProbeLossArgs), _P],
    'msdf_sampler_init': [C.POINTER(SamplerArgs), _P],
    'msdf_sampler_beta': [C.POINTER(SamplerArgs), _P],
    'msdf_sampler_resample': [C.POINTER(SamplerArgs), _P],
    'msdf_sampler_finish': [C.POINTER(SamplerArgs), _P],
    'msdf_sampler_error_bound': [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P],
    'msdf_laplace_density': [_P, _P, C.c_int, C.c_int64, C.c_int, _P, _P],
    'msdf_laplace_density_backward': [_P, _P, C.c_int, C.c_int64, C.c_int, _P, _P, _P, _P],
    'msdf_mc_workspace_bytes': [C.c_int, C.c_int, C.c_int],
    'msdf_mc_count': [_P, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P],
    'msdf_mc_emit': [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P, _P],
    'msdf_nn_split_count': [C.c_int64, C.c_int64, C.c_int],
    'msdf_nn_workspace_bytes': [C.c_int64, C.c_int64, C.c_int],
    'msdf_nn_search': [_P, C.c_int64, _P, C.c_int64, C.c_int, _P, _P, _P, _P],
    'msdf_voxel_keys': [_P, C.c_int64, _P, C.c_float, _P, _P],
    'msdf_voxel_mean': [_P, _P, _P, C.c_int64, C.c_int64, _P, _P],
    'msdf_raster_depth': [_P, C.c_int64, _P, C.c_int64, _P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                          C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _P, _P],
    'msdf_tsdf_integrate': [_P, _P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                            C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                            C.c_float, C.c_float, C.c_float, C.c_int, _P, _P, _P],
    'msdf_tsdf_face_keep': [_P, C.c_int64, _P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, _P, _P],
    'msdf_cull_vertices': [_P, C.c_int64, _P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                           _P, _P],
    'msdf_dtu_dilate_workspace_bytes': [C.c_int, C.c_int, C.c_int],
    'msdf_dtu_dilate': [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P],
    'msdf_dtu_mask_vertices': [_P, C.c_int64, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P],
    'msdf_dtu_lattice_count': [_P, C.c_int64, _P, C.c_int64, C.c_double, _P, _P],
    'msdf_dtu_lattice_emit': [_P, C.c_int64, _P, C.c_int64, C.c_double, _P, C.c_int64, _P, _P],
    'msdf_dtu_thin_workspace_bytes': [C.c_int64],
    'msdf_dtu_thin_keys': [_P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P],
    'msdf_dtu_thin_prepare': [_P, _P, _P, _P, C.c_int64, _P, _P],
    'msdf_dtu_thin_round': [_P, C.c_int64, C.c_double, _P, _P],
    'msdf_dtu_thin_finish': [_P, _P, C.c_int64, _P, _P],
}, 'monosdf_gridnn.h': {                                   # csrc/gridnn.hip
    'msdf_gnn_workspace_bytes': [C.c_int64],
    'msdf_gnn_cells': [_P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _P,
                       _P],
    'msdf_gnn_records': [_P, _P, C.c_int64, _P, _P],
    'msdf_gnn_query': [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_double, C.c_double, C.c_double, C.c_double,
                       C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P],
}, 'monosdf_meshcc.h': {                                   # csrc/meshcc.hip
    'msdf_mcc_edge_keys': [_P, C.c_int64, _P, _P],
    'msdf_mcc_init': [_P, C.c_int64, _P],
    'msdf_mcc_link_edges': [_P, _P, C.c_int64, C.c_int, _P, _P],
    'msdf_mcc_link_vertices': [_P, C.c_int64, _P, _P],
    'msdf_mcc_flatten': [_P, C.c_int64, _P],
    'msdf_mcc_segment_sum': [_P, _P, C.c_int64, _P, _P],
}, 'monosdf_obb.h': {                                      # csrc/obb.hip
    'msdf_obb_support_workspace_bytes': [C.c_int64, C.c_int64],
    'msdf_obb_support': [_P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P],
    'msdf_obb_candidates': [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, _P],
}, 'monosdf_highres.h': {                                  # csrc/highres.hip
    'msdf_hrc_workspace_bytes': [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64],
    'msdf_hrc_merge_depth': [_P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P],
    'msdf_hrc_merge_normals': [_P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P],
}, 'monosdf_icp.h': {                                      # csrc/icp.hip
    'msdf_icp_state_bytes': [C.c_int64],
    'msdf_icp_workspace_bytes': [C.c_int64],
    'msdf_icp_transform': [_P, C.c_int64, _P, _P, _P],
    'msdf_icp_accumulate': [_P, _P, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P],
    'msdf_icp_solve': [_P, C.c_int64, _P, C.c_int64, C.c_double, C.c_double, _P, _P],
}, 'monosdf_render.h': {                                   # csrc/meshrender.hip
    'msdf_rnd_visibility_workspace_bytes': [C.c_int64, C.c_int64, C.c_int64],
    'msdf_rnd_visibility': [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                            C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, _P, _P, _P, _P],
    'msdf_rnd_vertex_normals': [_P, C.c_int64, _P, C.c_int64, _P, _P, _P, _P],
    'msdf_rnd_shade': [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_float, C.c_float, C.c_float, C.c_float,
                       C.c_float, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_float, C.c_float, C.c_float, _P,
                       C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _P, _P],
    'msdf_rnd_depth_l1': [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P],
    'msdf_rnd_views_see': [_P, C.c_int64, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64,
                           C.c_int64, _P, _P],
}}

_ENTRIES = [name for table in _ABI.values() for name in table]
if len(_ENTRIES) != len(set(_ENTRIES)):
    raise ImportError('monosdf_amd: bound under two headers: %s'
                      % sorted(n for n in set(_ENTRIES) if _ENTRIES.count(n) > 1))

_lib = None


def headers():
    """The header files under include/ that declare the ABI, the versioned one first."""
    return list(_ABI)


def signatures(header):
    """{entry: argtypes} of one header of ``headers()``."""
    return _ABI[header]


def load():
    """Load the HIP library once; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'monosdf_amd: %s not found -- build it with `python __graft_entry__.py` or '
            '`make -C monosdf_amd/csrc` (there is no non-HIP fallback)' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for table in _ABI.values():
        for name, argtypes in table.items():
            fn = getattr(lib, name)        # AttributeError if the symbol is missing: intended
            fn.argtypes = argtypes
            fn.restype = C.c_int64 if name.endswith('_bytes') else C.c_int
    if lib.msdf_abi_version() != ABI_VERSION:
        raise RuntimeError('monosdf_amd: ABI version mismatch, rebuild the library')
    _lib = lib
    return lib


def exported_symbols():
    """The sorted entry points of the versioned header."""
    return sorted(_ABI[VERSIONED_HEADER])


# bench.py sets this to a dict to collect (start, end) HIP events per entry point; they are recorded on
# PyTorch's current stream, which is the stream every kernel is launched on (stream_ptr()).
PROFILE = None


# bench.py may restrict the timed entry points to this set (None = all): two events per call are not free
# (~0.2 ms per step for the ~45 calls of a training step), and the roofline needs the large kernels only.
PROFILE_NAMES = None


def call(name, *args):
    prof = PROFILE
    if prof is not None and PROFILE_NAMES is not None and name not in PROFILE_NAMES:
        prof = None
    if prof is not None:
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    status = getattr(load(), name)(*args)
    if prof is not None:
        e1.record()
        prof.setdefault(name, []).append((e0, e1))
    if status != 0:
        raise RuntimeError('%s failed: %s' % (name, _ERR.get(status, 'status %d' % status)))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def addr(t):
    """Device address of a tensor for a pointer field of an argument struct (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Binder:
    """One struct of the ABI, filled by field name -- the only way this package fills an argument struct or a record.

    Named: a name that is no field of the struct raises, and so does `pad_`.  Complete: launch() and bytes() raise
    until every field but `pad_` has been given at least once, so NULL pointers and zero scalars are written out
    (None, 0).  Kind-checked: a pointer field takes a tensor (its data_ptr()), None (NULL) or a Python int (an address:
    a workspace region, a run flag); a scalar field takes a number and neither a tensor nor None.  Owning: `held` maps
    every pointer field to what was bound to it, so a bound tensor lives as long as this object.  Device, dtype and
    contiguity of a tensor are the caller's business (some fields are read through strided views on purpose)."""

    _pointer = {}            # struct class -> {field: whether it is a pointer}, without pad_

    def __init__(self, struct, **fields):
        if struct not in self._pointer:
            self._pointer[struct] = {n: t is C.c_void_p for n, t in struct._fields_ if n != 'pad_'}
        self.struct, self.held = struct(), {}
        self._kinds = self._pointer[struct]
        self._unnamed = set(self._kinds)
        self._ref = C.byref(self.struct)
        self.bind(**fields)

    def bind(self, **fields):
        """Give fields their values; a field may be given again."""
        kinds, struct, held = self._kinds, self.struct, self.held
        for name, value in fields.items():
            pointer = kinds.get(name)
            if pointer is None:
                raise AttributeError('monosdf_amd: %s has no field %r that can be given' % (type(struct).__name__, name))
            if pointer:
                if hasattr(value, 'data_ptr'):
                    address = value.data_ptr()
                elif value is None or type(value) is int:
                    address = value
                else:
                    raise TypeError('monosdf_amd: %s.%s is a pointer: it takes a tensor, None or an address, not %r'
                                    % (type(struct).__name__, name, value))
                held[name], value = value, address
            elif value is None or hasattr(value, 'data_ptr'):
                raise TypeError('monosdf_amd: %s.%s is a scalar: it takes a number, not %s'
                                % (type(struct).__name__, name, 'None' if value is None else 'a tensor'))
            setattr(struct, name, value)
        self._unnamed.difference_update(fields)

    def complete(self):
        """The struct, once every field has been named."""
        if self._unnamed:
            raise RuntimeError('monosdf_amd: %s with fields never given: %s'
                               % (type(self.struct).__name__, ', '.join(sorted(self._unnamed))))
        return self.struct

    def __bytes__(self):
        return bytes(self.complete())

    def launch(self, entry, plan=None, stream=None):
        """call(entry, [byref(plan),] byref(struct), stream); stream: a stream_ptr() taken earlier (default: now)."""
        self.complete()
        stream = stream_ptr() if stream is None else stream
        if plan is None:
            call(entry, self._ref, stream)
        else:
            call(entry, C.byref(plan), self._ref, stream)
