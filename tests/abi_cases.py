"""The C ABI as its headers state it, for tests/test_abi_cpu.py: one parser of the prototypes, one rule from a C
parameter to the ctypes types that may bind it, and per header under include/ what is expected of it."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
VERSIONED = 'monosdf_hip.h'

# The additive headers: the prefix of their names, their source file, whether that file is built with
# -ffp-contract=off, and their entry points; where it applies, `named_in`: the other headers whose text may name these
# entry points, and `depends`: further headers under csrc/ that the source shares with other sources.  The versioned
# header has no list of names here: its count is stated below, and the features that extended it keep their own
# subsets (test_dtu_cpu, test_refuse_cpu, test_mesh_eval_cpu).
VERSIONED_COUNT = 64
ADDITIVE = {
    'monosdf_gridnn.h': dict(prefix='msdf_gnn_', source='gridnn', no_contraction=True, named_in=('monosdf_icp.h',),
                             entries=('msdf_gnn_workspace_bytes', 'msdf_gnn_cells', 'msdf_gnn_records',
                                      'msdf_gnn_query')),
    'monosdf_meshcc.h': dict(prefix='msdf_mcc_', source='meshcc', no_contraction=False, entries=(
        'msdf_mcc_edge_keys', 'msdf_mcc_init', 'msdf_mcc_link_edges', 'msdf_mcc_link_vertices', 'msdf_mcc_flatten',
        'msdf_mcc_segment_sum')),
    'monosdf_obb.h': dict(prefix='msdf_obb_', source='obb', no_contraction=True, entries=(
        'msdf_obb_support_workspace_bytes', 'msdf_obb_support', 'msdf_obb_candidates')),
    'monosdf_highres.h': dict(prefix='msdf_hrc_', source='highres', no_contraction=True, entries=(
        'msdf_hrc_workspace_bytes', 'msdf_hrc_merge_depth', 'msdf_hrc_merge_normals')),
    'monosdf_icp.h': dict(prefix='msdf_icp_', source='icp', no_contraction=True, entries=(
        'msdf_icp_state_bytes', 'msdf_icp_workspace_bytes', 'msdf_icp_transform', 'msdf_icp_accumulate',
        'msdf_icp_solve')),
    'monosdf_render.h': dict(prefix='msdf_rnd_', source='meshrender', no_contraction=True, depends=('raster_core.h',),
                             entries=('msdf_rnd_visibility_workspace_bytes', 'msdf_rnd_visibility',
                                      'msdf_rnd_vertex_normals', 'msdf_rnd_shade', 'msdf_rnd_depth_l1',
                                      'msdf_rnd_views_see')),
}

C_SCALARS = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64,
             'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float, 'double': ctypes.c_double}
# entry points that take a struct pointer as an opaque address: a table in device memory
DEVICE_TABLES = {'msdf_pack_weights', 'msdf_weightnorm_forward', 'msdf_weightnorm_backward', 'msdf_wgrad',
                 'msdf_reduce'}


def mirrors():
    """C struct name -> its ctypes mirror: all fifteen structs of the ABI."""
    from monosdf_amd import _lib
    return {'msdf_plan_t': _lib.Plan, 'msdf_layer_t': _lib.Layer, 'msdf_packrule_t': _lib.PackRule,
            'msdf_wgrad_item_t': _lib.WgradItem, 'msdf_reduce_rule_t': _lib.ReduceRule,
            'msdf_fg_args_t': _lib.FgArgs, 'msdf_bw_args_t': _lib.BwArgs,
            'msdf_color_fwd_args_t': _lib.ColorFwdArgs, 'msdf_color_bwd_args_t': _lib.ColorBwdArgs,
            'msdf_composite_args_t': _lib.CompositeArgs, 'msdf_composite_bwd_args_t': _lib.CompositeBwdArgs,
            'msdf_sampler_args_t': _lib.SamplerArgs, 'msdf_wn_layer_t': _lib.WnLayer,
            'msdf_probe_loss_args_t': _lib.ProbeLossArgs, 'msdf_monosdf_loss_args_t': _lib.MonoSdfLossArgs}


def header_text(header):
    return open(os.path.join(INCLUDE, header)).read()


def prototypes(header):
    """(return type, name, parameter text) of every prototype of a header under include/, both comment forms
    stripped."""
    text = re.sub(r'/\*.*?\*/', ' ', header_text(header), flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    return re.findall(r'^(int|int64_t) (msdf_\w+)\((.*?)\);', text, flags=re.M | re.S)


def parameters(params):
    """The parameter text of a prototype -> per parameter its words, '*' a word of its own; ``(void)`` -> none."""
    words = [p.split() for p in params.replace('*', ' * ').split(',')]
    return [] if words == [['void']] else words


def accepted_argtypes(name, params):
    """Per parameter the ctypes types that may bind it: a scalar has one; a pointer to a mirrored struct is
    POINTER(mirror), or an address where the entry takes a table of such structs in device memory (DEVICE_TABLES);
    every other pointer is an address."""
    structs, accepted = mirrors(), []
    for i, words in enumerate(parameters(params)):
        words = [w for w in words[:-1] if w != 'const']            # the last word is the parameter's name
        if words[-1] != '*':
            assert len(words) == 1, (name, i, words)
            accepted.append((C_SCALARS[words[0]],))
        elif words[0] in structs:
            assert len(words) == 2, (name, i, words)
            accepted.append((ctypes.POINTER(structs[words[0]]), ctypes.c_void_p))
        else:
            assert not words[0].startswith('msdf_'), (name, i, words)      # T*, T* const*: an address
            accepted.append((ctypes.c_void_p,))
    return accepted
