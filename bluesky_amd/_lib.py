"""ctypes binding of ``libbsaccel.so`` (declarations in ``include/bsaccel.h``).

The HIP library is the ONLY compute path: if it is missing, or no HIP device
is visible, every call raises ``AccelUnavailable`` -- there is deliberately no
CPU fallback in the product path.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BSACCEL_LIB', os.path.join(_HERE, 'libbsaccel.so'))

ABI_VERSION = 2
PF_BLOCK_PAIRS = 512   # BSA_PF_BLOCK_PAIRS: stage-1 pair tests per swept prefilter block
FLAG_WITH_DCPA = 1
FLAG_NOPRUNE = 2
FLAG_RESORT = 4
FLAG_KWIK = 8
FLAG_STAGE1_T0 = 16
GEO_KWIK = 1
GEO_PAIRWISE = 2

_c_dp = ctypes.POINTER(ctypes.c_double)
_c_fp = ctypes.POINTER(ctypes.c_float)
_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_u8p = ctypes.POINTER(ctypes.c_uint8)
_c_i64p = ctypes.POINTER(ctypes.c_int64)
_c_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p


class AccelUnavailable(RuntimeError):
    """libbsaccel.so could not be loaded or has no usable HIP device."""


class AccelError(RuntimeError):
    """A libbsaccel call returned an error status."""


# name -> (restype, argtypes); must match include/bsaccel.h exactly
SIGNATURES = {
    'bsa_abi_version': (ctypes.c_int, []),
    'bsa_device_count': (ctypes.c_int, []),
    'bsa_create': (_vp, [ctypes.c_int]),
    'bsa_destroy': (None, [_vp]),
    'bsa_last_error': (ctypes.c_char_p, [_vp]),
    'bsa_sync': (ctypes.c_int, [_vp]),
    'bsa_set_state': (ctypes.c_int, [_vp, ctypes.c_int64] + [_c_dp] * 6),
    'bsa_set_intruder': (ctypes.c_int, [_vp, ctypes.c_int64] + [_c_dp] * 6),
    'bsa_detect': (ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_int, ctypes.c_int64, ctypes.c_int64, _c_i64p, _c_i64p]),
    'bsa_fetch_pairs': (ctypes.c_int, [_vp, _c_i32p, _c_i32p, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp,
                                       _c_i32p, _c_i32p, _c_u8p, _c_dp]),
    'bsa_last_candidates': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_last_tiles': (ctypes.c_int, [_vp, _c_i64p, _c_i64p, _c_i64p]),
    'bsa_set_candidate_reuse': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    'bsa_reuse_stats': (ctypes.c_int, [_vp, _c_i64p, _c_i64p]),
    'bsa_set_tile_reuse': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    'bsa_tile_reuse_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_set_hk': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double]),
    'bsa_hk_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_set_halo_overlap': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bsa_halo_overlap_count': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_reuse_budget_use': (ctypes.c_int, [_vp, _c_dp]),
    'bsa_last_timings': (ctypes.c_int, [_vp, _c_dp]),
    'bsa_timing_reset': (ctypes.c_int, [_vp]),
    'bsa_set_candidate_capacity': (ctypes.c_int, [_vp, ctypes.c_int64]),
    'bsa_timing_summary': (ctypes.c_int, [_vp, _c_dp, _c_i64p]),
    'bsa_set_timing_sample': (ctypes.c_int, [_vp, ctypes.c_int]),
}

PRIO_CODES = {'FF1': 1, 'FF2': 2, 'FF3': 3, 'LAY1': 4, 'LAY2': 5}


class MvpParams(ctypes.Structure):
    """bsa_mvp_params (include/bsaccel.h)."""
    _fields_ = [('Rm', ctypes.c_double), ('dhm', ctypes.c_double),
                ('dtlookahead', ctypes.c_double), ('vmin', ctypes.c_double),
                ('vmax', ctypes.c_double), ('vsmin', ctypes.c_double), ('vsmax', ctypes.c_double),
                ('swresohoriz', ctypes.c_int32), ('swresospd', ctypes.c_int32),
                ('swresohdg', ctypes.c_int32), ('swresovert', ctypes.c_int32),
                ('swprio', ctypes.c_int32), ('priocode', ctypes.c_int32),
                ('swnoreso', ctypes.c_int32), ('swresooff', ctypes.c_int32)]


class KinIO(ctypes.Structure):
    """bsa_kin_io (include/bsaccel.h)."""
    _fields_ = [(k, _c_dp) for k in ('ptas', 'phdg', 'palt', 'pvs', 'bank', 'eps', 'accel',
                                     'tas', 'hdg', 'alt', 'vs', 'lat', 'lon', 'ax', 'delspd',
                                     'cas', 'mach', 'gsnorth', 'gseast', 'gs', 'trk', 'coslat',
                                     'az')] + [('swhdgsel', _c_u8p), ('swaltsel', _c_u8p)]


SIGNATURES.update({
    'bsa_set_pairs': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i32p, _c_i32p, _c_dp, _c_dp, _c_dp,
                                     _c_dp]),
    'bsa_mvp': (ctypes.c_int, [_vp, ctypes.POINTER(MvpParams), _c_dp, _c_dp, _c_dp, _c_dp, _c_u8p,
                               _c_u8p, _c_dp, _c_dp, _c_dp, _c_dp, _c_fp, _c_fp]),
    'bsa_kinematics': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_double, ctypes.c_int,
                                      ctypes.c_double, ctypes.c_double, ctypes.POINTER(KinIO)]),
})

class SimParams(ctypes.Structure):
    """bsa_sim_params (include/bsaccel.h)."""
    _fields_ = [('simdt', ctypes.c_double), ('rpz', ctypes.c_double), ('hpz', ctypes.c_double),
                ('tla', ctypes.c_double), ('cd_every', ctypes.c_int32), ('reso', ctypes.c_int32),
                ('mvp', MvpParams), ('winddim', ctypes.c_int32), ('resume_nav', ctypes.c_int32),
                ('windnorth', ctypes.c_double), ('windeast', ctypes.c_double)]


SIM_STATE_FIELDS = ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'gs', 'trk', 'gseast', 'gsnorth',
                    'ap_trk', 'ap_tas', 'ap_alt', 'ap_vs', 'selalt', 'bank', 'eps', 'accel',
                    'asas_alt')
SIM_OUT_FIELDS = ('lat', 'lon', 'alt', 'tas', 'hdg', 'vs', 'gs', 'trk', 'gseast', 'gsnorth',
                  'asas_trk', 'asas_tas', 'asas_vs', 'asas_alt')


class SimState(ctypes.Structure):
    """bsa_sim_state (include/bsaccel.h)."""
    _fields_ = [(k, _c_dp) for k in SIM_STATE_FIELDS]


class SimOut(ctypes.Structure):
    """bsa_sim_out (include/bsaccel.h)."""
    _fields_ = [(k, _c_dp) for k in SIM_OUT_FIELDS] + [('active', _c_u8p)]


ACDATA_F64 = ('lat', 'lon', 'alt', 'tas', 'cas', 'gs', 'trk', 'vs', 'tcpamax')
ACDATA_COUNTS = ('nconf_cur', 'nconf_tot', 'nlos_cur', 'nlos_tot')


class AcData(ctypes.Structure):
    """bsa_acdata (include/bsaccel.h)."""
    _fields_ = ([(k, ctypes.c_int64) for k in ('steps', 'row_begin', 'row_end') + ACDATA_COUNTS] +
                [(k, _c_dp) for k in ACDATA_F64] + [('inconf', _c_u8p), ('asasn', _c_fp), ('asase', _c_fp)])


class PairsOut(ctypes.Structure):
    """bsa_pairs_out (include/bsaccel.h)."""
    _fields_ = [('ci', _c_i32p), ('cj', _c_i32p), ('qdr', _c_dp), ('dist', _c_dp), ('tcpa', _c_dp),
                ('tinconf', _c_dp), ('dcpa', _c_dp), ('li', _c_i32p), ('lj', _c_i32p), ('inconf', _c_u8p),
                ('tcpamax', _c_dp)]


SIGNATURES.update({
    'bsa_group_create': (_vp, [ctypes.c_int]),
    'bsa_group_destroy': (None, [_vp]),
    'bsa_comm_init_group': (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    'bsa_gather_counts': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_gather_pairs': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(PairsOut)]),
    'bsa_comm_unique_id': (ctypes.c_int, [ctypes.c_char_p]),
    'bsa_comm_init': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    'bsa_comm_allreduce_max': (ctypes.c_int, [_vp, _c_dp, ctypes.c_int]),
    'bsa_comm_allreduce_sum': (ctypes.c_int, [_vp, _c_dp, ctypes.c_int]),
    'bsa_comm_info': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    'bsa_sim_init': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(SimState),
                                    ctypes.POINTER(SimParams)]),
    'bsa_sim_step': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bsa_sim_update': (ctypes.c_int, [_vp, ctypes.POINTER(SimState)]),
    'bsa_sim_create': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(SimState)]),
    'bsa_sim_delete': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i64p]),
    'bsa_sim_read': (ctypes.c_int, [_vp, ctypes.POINTER(SimOut)]),
    'bsa_sim_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_sim_row_ids': (ctypes.c_int, [_vp, _c_i32p]),
    'bsa_set_row_bucket': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bsa_sim_detect_rows': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _c_i64p, _c_i64p]),
    'bsa_sim_asas_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_sim_resopairs': (ctypes.c_int, [_vp, _c_i32p, _c_i32p, ctypes.c_int64, _c_i64p]),
    'bsa_qdrdist': (ctypes.c_int, [_vp, ctypes.c_int64, _c_dp, _c_dp, ctypes.c_int64, _c_dp, _c_dp,
                                   ctypes.c_int, _c_dp, _c_dp]),
    'bsa_geo_last_ms': (ctypes.c_int, [_vp, _c_dp]),
    'bsa_sim_acdata_request': (ctypes.c_int, [_vp]),
    'bsa_set_windfield': (ctypes.c_int, [_vp, ctypes.c_int64, _c_dp, _c_dp, _c_dp, _c_dp]),
    'bsa_set_windfield3d': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_double,
                                           _c_dp, _c_dp, _c_dp, _c_dp]),
    'bsa_wind_getdata': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp]),
    'bsa_sim_set_limits': (ctypes.c_int, [_vp] + [_c_dp] * 6),
    'bsa_sim_set_perf': (ctypes.c_int, [_vp, ctypes.c_int64, _c_dp, _c_i32p]),
    'bsa_sim_read_perf': (ctypes.c_int, [_vp, _c_u8p, _c_dp]),
    'bsa_sim_acdata_poll': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(AcData)]),
})



class AsasOut(ctypes.Structure):
    """bsa_asas_out (include/bsaccel.h)."""
    _fields_ = [(k, _c_dp) for k in ('trk', 'tas', 'vs', 'alt')] + [('asase', _c_fp), ('asasn', _c_fp),
                                                                   ('active', _c_u8p), ('dropped', _c_u8p)]


SIGNATURES.update({
    'bsa_sim_cd': (ctypes.c_int, [_vp]),
    'bsa_sim_set_params': (ctypes.c_int, [_vp, ctypes.POINTER(SimParams)]),
    'bsa_sim_set_reso_lists': (ctypes.c_int, [_vp, _c_u8p, _c_u8p]),
    'bsa_sim_read_asas': (ctypes.c_int, [_vp, ctypes.POINTER(AsasOut)]),
    'bsa_sim_halo_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_sim_set_halo_cap': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64]),
    'bsa_sim_halo_recheck': (ctypes.c_int, [_vp]),
    'bsa_sim_probe_rank': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    'bsa_set_exact_fusion': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    'bsa_exact_fusion_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_set_symmetric_sweep': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bsa_symmetric_sweep_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_set_lean_pairs': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bsa_lean_pairs_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_listed_items': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64, _c_i64p]),
    'bsa_sim_comm_stats': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_sim_set_atmos': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bsa_sim_read_atmos': (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp]),
    'bsa_openap_forces': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _c_dp, _c_dp, _c_i32p, _c_u8p] +
                          [_c_dp] * 10),
    'bsa_sim_set_forces': (ctypes.c_int, [_vp, ctypes.c_int64, _c_dp, _c_dp]),
    'bsa_sim_read_forces': (ctypes.c_int, [_vp] + [_c_dp] * 7),
})

FORCE_OUTPUTS = ('cd0', 'drag', 'thrustratio', 'thrust', 'fuelflow', 'bank')

FMS_TRAFFIC = ('lat', 'lon', 'alt', 'tas', 'gs', 'trk', 'ax', 'bank')
FMS_REALS = ('actwp_lat', 'actwp_lon', 'actwp_nextaltco', 'actwp_xtoalt', 'actwp_spd', 'actwp_vs',
             'actwp_turndist', 'actwp_flyby', 'actwp_next_qdr', 'dist2vs', 'vnavvs', 'swvnavvs', 'selspd',
             'selvs', 'apvsdef')
FMS_FLAGS = ('swlnav', 'swvnav', 'abco', 'belco')
FMS_TARGETS = ('ap_trk', 'ap_tas', 'ap_alt', 'ap_vs', 'selalt')
ROUTE_COLS = 8


class FmsState(ctypes.Structure):
    """bsa_fms_state (include/bsaccel.h)."""
    _fields_ = [(k, _c_dp) for k in FMS_REALS] + [(k, _c_u8p) for k in FMS_FLAGS]


class SimCreateExtra(ctypes.Structure):
    """bsa_sim_create_extra (include/bsaccel.h)."""
    _fields_ = ([(k, _c_dp) for k in ('hmax', 'vmin', 'vmax', 'vsmin', 'vsmax', 'axmax')] +
                [('type_idx', _c_i32p), ('mass', _c_dp), ('nrows', ctypes.c_int64), ('route_rows', _c_dp),
                 ('rt_off', _c_i32p), ('rt_n', _c_i32p), ('iactwp', _c_i32p), ('st', ctypes.POINTER(FmsState))])


class RouteEditRec(ctypes.Structure):
    """bsa_route_edit_rec (include/bsaccel.h)."""
    _fields_ = ([(k, ctypes.c_int32) for k in ('aircraft', 'op', 'pos', 'flyby', 'wptype', 'bump_active')] +
                [(k, ctypes.c_double) for k in ('lat', 'lon', 'alt', 'spd')])


ROUTE_REC_DTYPE = np.dtype([(k, np.int32) for k in ('aircraft', 'op', 'pos', 'flyby', 'wptype', 'bump_active')] +
                           [(k, np.float64) for k in ('lat', 'lon', 'alt', 'spd')])
ROUTE_INSERT, ROUTE_OVERWRITE, ROUTE_DELETE, ROUTE_DIRECT = range(4)
ROUTE_ERRORS = {1: 'aircraft index out of range', 2: 'no such op', 3: 'pos outside the route',
                4: 'runway / calculated waypoint', 5: 'lat / lon not finite', 6: 'guidance on several ranks'}
_c_recp = ctypes.POINTER(RouteEditRec)


class RouteEditRefused(ValueError):
    """A route edit batch was refused (nothing changed); ``code``: BSA_ROUTE_ERR_*."""

    def __init__(self, code, msg):
        ValueError.__init__(self, msg)
        self.code = code


def route_records(records):
    """A batch of edit records as a contiguous ROUTE_REC_DTYPE array (from such an
    array, or a list of dicts / tuples in the field order)."""
    if isinstance(records, np.ndarray) and records.dtype == ROUTE_REC_DTYPE:
        return np.ascontiguousarray(records).ravel()
    out = np.zeros(len(records), ROUTE_REC_DTYPE)
    for q, r in enumerate(records):
        if isinstance(r, dict):
            for k in ROUTE_REC_DTYPE.names:
                out[q][k] = r.get(k, 0)
        else:
            out[q] = tuple(r)
    return out


SIGNATURES.update({
    'bsa_route_edit': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _c_dp, _c_u8p, _c_i32p, _c_i32p, _c_i32p] +
                       [_c_dp] * 7 + [ctypes.POINTER(FmsState), _c_dp, ctypes.c_int64, _c_recp, ctypes.c_int64, _c_dp,
                                      _c_u8p, _c_i32p, _c_i32p, _c_i64p]),
    'bsa_sim_route_edit': (ctypes.c_int, [_vp, ctypes.c_int64, _c_recp]),
    'bsa_sim_route_rows': (ctypes.c_int, [_vp, _c_i64p]),
    'bsa_sim_read_routes': (ctypes.c_int, [_vp, ctypes.c_int64, _c_dp, _c_u8p, _c_i32p, _c_i32p, _c_i64p]),
    'bsa_sim_route_stats': (ctypes.c_int, [_vp] + [_c_i64p] * 4),
    'bsa_sim_create_with': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(SimState),
                                           ctypes.POINTER(SimCreateExtra)]),
    'bsa_fms_update': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _c_dp, _c_i32p, _c_i32p, _c_i32p] +
                       [_c_dp] * 8 + [ctypes.POINTER(FmsState)] + [_c_dp] * 5),
    'bsa_sim_set_fms': (ctypes.c_int, [_vp, ctypes.c_int64, _c_dp, _c_i32p, _c_i32p, _c_i32p, ctypes.POINTER(FmsState),
                                       ctypes.c_double, ctypes.c_double]),
    'bsa_sim_read_fms': (ctypes.c_int, [_vp, ctypes.POINTER(FmsState), _c_i32p] + [_c_dp] * 7 + [_c_i64p]),
    'bsa_fms_recover': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _c_dp, _c_i32p, _c_i32p, _c_i32p] +
                        [_c_dp] * 7 + [ctypes.POINTER(FmsState), _c_dp, _c_i32p]),
    'bsa_sim_set_recovery': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bsa_sim_read_dropcount': (ctypes.c_int, [_vp, _c_i32p]),
    'bsa_turb_draws': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                      _c_u64p, _c_dp]),
    'bsa_turb_apply': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_double] + [_c_dp] * 4 +
                       [ctypes.c_uint64, ctypes.c_uint64] + [_c_dp] * 5),
    'bsa_sim_set_turbulence': (ctypes.c_int, [_vp, ctypes.c_int, _c_dp, ctypes.c_uint64]),
    'bsa_sim_turb_call': (ctypes.c_int, [_vp, _c_i64p, _c_i64p]),
    'bsa_cond_update': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i32p, _c_i32p, _c_dp, _c_dp, ctypes.c_int64, _c_dp, _c_dp,
                                       _c_i32p, _c_i64p]),
    'bsa_sim_set_conditions': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i32p, _c_i32p, _c_dp, _c_dp]),
    'bsa_sim_steps_run': (ctypes.c_int, [_vp, _c_i64p, _c_i64p]),
    'bsa_sim_cond_poll': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i32p, _c_i64p, _c_i64p]),
    'bsa_sim_read_conditions': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i32p, _c_i32p, _c_dp, _c_dp, _c_i64p]),
})

AREA_TYPES = {'LINE': 0, 'BOX': 1, 'CIRCLE': 2, 'POLY': 3}
AREA_NOCULL = 1
AREA_SHAPES_MAX = 1024
AREA_VERTS_MAX = 65536


class AreaShape(ctypes.Structure):
    """bsa_area_shape (include/bsaccel.h)."""
    _fields_ = [('type', ctypes.c_int32), ('nvert', ctypes.c_int32), ('voff', ctypes.c_int64),
                ('top', ctypes.c_double), ('bottom', ctypes.c_double), ('c', ctypes.c_double * 4),
                ('blat', ctypes.c_double * 2), ('blon', ctypes.c_double * 2)]


def area_table(areas):
    """(AreaShape array, vertices (nvert, 2) fp64) of ``areas``: a sequence of
    ``(type, coordinates, top, bottom)`` with the reference's coordinate lists (areafilter.py:15-24):
    BOX lat0 lon0 lat1 lon1; CIRCLE clat clon r [NM]; POLY* lat lon lat lon ...; LINE anything."""
    tab = (AreaShape * max(1, len(areas)))()
    verts = []
    nv = 0
    for k, (typ, coords, top, bottom) in enumerate(areas):
        t = 'POLY' if str(typ)[:4] == 'POLY' else str(typ)
        if t not in AREA_TYPES:
            raise ValueError('unknown area type %r' % (typ,))
        sh = tab[k]
        sh.type, sh.top, sh.bottom = AREA_TYPES[t], float(top), float(bottom)
        co = f64(coords).ravel()
        need = {'BOX': 4, 'CIRCLE': 3}.get(t, 0)
        if len(co) < need:
            raise ValueError('%s needs %d coordinates' % (t, need))
        for q in range(need):
            sh.c[q] = co[q]
        if t == 'POLY':
            v = co[:2 * (len(co) // 2)].reshape(-1, 2)   # areafilter.py:97
            sh.nvert, sh.voff = len(v), nv
            verts.append(v)
            nv += len(v)
    verts = np.ascontiguousarray(np.concatenate(verts)) if verts else np.zeros((0, 2))
    return tab, verts


SIGNATURES.update({
    'bsa_area_inside': (ctypes.c_int, [_vp, ctypes.c_int64, _c_dp, _c_dp, _c_dp, ctypes.c_int64,
                                       ctypes.POINTER(AreaShape), ctypes.c_int64, _c_dp, ctypes.c_int,
                                       _c_u64p, _c_u64p]),
    'bsa_sim_set_areas': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(AreaShape), ctypes.c_int64, _c_dp]),
    'bsa_sim_set_sectors': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i32p, ctypes.c_int64]),
    'bsa_sim_sectors_poll': (ctypes.c_int, [_vp] + [_c_u64p] * 5 + [_c_i64p, _c_i64p, _c_u64p, _c_u64p]),
    'bsa_sim_sectors_deleted': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i64p, _c_u64p, _c_i64p]),
    'bsa_exparea_update': (ctypes.c_int, [_vp, ctypes.c_int64] + [_c_dp] * 10 + [_c_u8p, ctypes.c_double,
                                          ctypes.POINTER(AreaShape), ctypes.c_int64, _c_dp, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_double, _c_i32p, _c_i64p, _c_i32p, _c_i64p]),
    'bsa_sim_set_exparea': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int32, ctypes.c_double, ctypes.c_int64,
                                           ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    'bsa_sim_exparea_simt': (ctypes.c_int, [_vp, ctypes.c_double]),
    'bsa_sim_exparea_poll': (ctypes.c_int, [_vp, ctypes.c_int64, _c_i32p, _c_i64p, _c_i32p, _c_i64p, _c_dp, _c_i64p]),
    'bsa_sim_read_exparea': (ctypes.c_int, [_vp] + [_c_dp] * 5 + [_c_u8p]),
    'bsa_trails_update': (ctypes.c_int, [_vp, ctypes.c_int64] + [_c_dp] * 5 + [ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                         ctypes.c_int64] + [_c_dp] * 5 + [_c_i32p, _c_i64p]),
    'bsa_sim_set_trails': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _c_dp,
                                          ctypes.c_int64]),
    'bsa_sim_trails_drain': (ctypes.c_int, [_vp, ctypes.c_int64] + [_c_dp] * 5 + [_c_i32p, _c_i64p, _c_dp, _c_dp]),
    'bsa_sim_read_trails': (ctypes.c_int, [_vp, _c_dp, _c_dp, _c_dp, _c_dp, _c_dp, _c_i64p]),
    'bsa_adsb_draws': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                      _c_u64p, _c_dp, _c_dp]),
    'bsa_adsb_update': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_int, _c_dp,
                                       ctypes.c_int, _c_dp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64] + [_c_dp] * 15),
    'bsa_sim_set_adsb': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _c_dp, ctypes.c_double, ctypes.c_uint64,
                                        ctypes.c_int, ctypes.c_double, _c_dp]),
    'bsa_sim_read_adsb': (ctypes.c_int, [_vp] + [_c_dp] * 9 + [_c_i64p]),
    'bsa_sim_adsb_call': (ctypes.c_int, [_vp, _c_i64p, _c_i64p]),
    'bsa_sim_aborts': (ctypes.c_int, [_vp, _c_i64p]),
})

# the ADS-B picture's arrays beside lastupdate (adsbmodel.py:16-23), and bsa_adsb_update's draw modes
ADSB_FIELDS = ('lat', 'lon', 'alt', 'trk', 'tas', 'gs', 'vs')
ADSB_DRAWS = ('shared', 'per_aircraft')

# one record of bsa_sim_exparea_poll (fp64 words, per exited aircraft)
EXPAREA_RECORD = ('create_time', 'distance2D', 'distance3D', 'work', 'lat', 'lon', 'alt', 'tas', 'vs', 'hdg', 'active',
                  'ap_alt', 'ap_tas', 'ap_vs', 'ap_trk', 'asas_alt', 'asas_tas', 'asas_vs', 'asas_trk')

GEOVEC_GSMIN, GEOVEC_GSMAX, GEOVEC_TRK, GEOVEC_VSMIN, GEOVEC_VSMAX = 1, 2, 4, 8, 16
GEOVEC_MAX = 256
GEOVEC_TARGETS = ('selspd', 'ap_trk', 'selvs', 'selalt')


class Geovec(ctypes.Structure):
    """bsa_geovec (include/bsaccel.h)."""
    _fields_ = [('shape', ctypes.c_int32), ('given', ctypes.c_int32)] + \
               [(k, ctypes.c_double) for k in ('gsmin', 'gsmax', 'trkmin', 'trkmax', 'vsmin', 'vsmax')]


def geovec_rows(rows):
    """A ``Geovec`` array of ``rows``: such an array already, or a sequence of
    ``(shape, given, gsmin, gsmax, trkmin, trkmax, vsmin, vsmax)``."""
    if isinstance(rows, ctypes.Array) and getattr(rows, '_type_', None) is Geovec:
        return rows, len(rows)
    tab = (Geovec * max(1, len(rows)))()
    for k, r in enumerate(rows):
        tab[k] = Geovec(int(r[0]), int(r[1]), *[float(x) for x in r[2:8]])
    return tab, len(rows)


SIGNATURES.update({
    'bsa_geovec_apply': (ctypes.c_int, [_vp, ctypes.c_int64] + [_c_dp] * 5 +
                         [ctypes.c_int64, ctypes.POINTER(AreaShape), ctypes.c_int64, _c_dp,
                          ctypes.c_int64, ctypes.POINTER(Geovec), ctypes.c_int] + [_c_dp] * 4 + [_c_u64p]),
    'bsa_sim_set_geovectors': (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(Geovec), ctypes.c_int64]),
    'bsa_sim_geovec_stats': (ctypes.c_int, [_vp, _c_i64p, _c_u64p]),
})

# the tests' entries to the device scan and the ordered index list
_c_u32p = ctypes.POINTER(ctypes.c_uint32)
SIGNATURES.update({
    'bsa_scan_excl': (ctypes.c_int, [_vp, ctypes.c_int64, _c_u32p, _c_u32p]),
    'bsa_flagged_list': (ctypes.c_int, [_vp, ctypes.c_int64, _c_u8p, _c_u32p, ctypes.c_uint32, ctypes.c_int64, _c_i32p,
                                        _c_i64p]),
})

UNIQUE_ID_BYTES = 128

_lib = None
_lib_lock = threading.Lock()


def load(path=None):
    """Load and type the library (idempotent).  Raises AccelUnavailable."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise AccelUnavailable('libbsaccel.so not built (%s); run `make -C bluesky_amd/csrc` '
                                   'or __graft_entry__.build()' % p)
        try:
            lib = ctypes.CDLL(p)
        except OSError as e:
            raise AccelUnavailable('cannot load %s: %s' % (p, e))
        skipped = []
        for name, (res, args) in SIGNATURES.items():
            if not hasattr(lib, name) and p != os.path.join(_HERE, 'libbsaccel.so') \
                    and os.environ.get('BSACCEL_AB') == '1':
                skipped.append(name)   # an older build selected for an A/B measurement
                continue
            if not hasattr(lib, name):
                raise AccelUnavailable('%s lacks %s (stale build? set BSACCEL_AB=1 to load an older '
                                       'build for an A/B measurement)' % (p, name))
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        if skipped:
            import sys
            print('[bsaccel] %s: %d symbols missing (BSACCEL_AB=1): %s' % (p, len(skipped), ' '.join(skipped)),
                  file=sys.stderr)
        v = lib.bsa_abi_version()
        if v != ABI_VERSION:
            raise AccelUnavailable('ABI mismatch: library %d, bindings %d' % (v, ABI_VERSION))
        _lib = lib
        return lib


def mapped_library():
    """(path, sha256) of the libbsaccel this process actually mapped (from
    /proc/self/maps; measurement provenance: bench.py / tools/pmc_roofline.py)."""
    import hashlib
    load()
    path = None
    try:
        with open('/proc/self/maps') as f:
            for line in f:
                q = line.split()
                if len(q) >= 6 and os.path.basename(q[-1]).startswith('libbsaccel'):
                    path = q[-1]
                    break
    except OSError:
        pass
    path = path or os.path.realpath(LIB_PATH)
    with open(path, 'rb') as f:
        return path, hashlib.sha256(f.read()).hexdigest()


def comm_unique_id():
    """128-byte RCCL communicator id (create on one rank, ship to the others)."""
    lib = load()
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    if lib.bsa_comm_unique_id(buf) != 0:
        raise AccelError('bsa_comm_unique_id failed')
    return buf.raw


class Group:
    """In-process group of contexts (bsa_group_*): the ranks of a row-sharded
    sim in ONE process, one host thread per rank.  Keep it alive until every
    member context is closed."""

    def __init__(self, nranks):
        self.lib = load()
        self.h = self.lib.bsa_group_create(int(nranks))
        if not self.h:
            raise AccelError('bsa_group_create(%d) failed' % nranks)
        self.nranks = nranks

    def close(self):
        if getattr(self, 'h', None):
            self.lib.bsa_group_destroy(self.h)
            self.h = None


def ptr(a, ctype=_c_dp):
    return None if a is None else a.ctypes.data_as(ctype)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Context:
    """One HIP device + stream + its device buffers (bsa_ctx)."""

    def __init__(self, device=0):
        self.lib = load()
        ndev = self.lib.bsa_device_count()
        if ndev <= 0:
            raise AccelUnavailable('no HIP device visible (bsa_device_count=%d)' % ndev)
        h = self.lib.bsa_create(int(device))
        if not h:
            raise AccelUnavailable('bsa_create(%d) failed: %s'
                                   % (device, self.lib.bsa_last_error(None).decode()))
        self.h = h
        self.device = device
        # bumped by every call that replaces the device-resident state or pairs
        # (set_state / set_intruder / detect / set_pairs / sim_*): the MVP drop-in
        # reuses a detect's device pairs only while it is unchanged
        self.gen = 0

    def close(self):
        if getattr(self, 'h', None):
            self.lib.bsa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, status, what):
        if status != 0:
            raise AccelError('%s: %s' % (what, self.lib.bsa_last_error(self.h).decode()))

    # ---------------------------------------------------------------- state
    def set_state(self, lat, lon, trk, gs, alt, vs):
        self.gen += 1
        arrs = [f64(x) for x in (lat, lon, trk, gs, alt, vs)]
        n = len(arrs[0])
        if any(len(a) != n for a in arrs):
            raise ValueError('state arrays differ in length')
        self.check(self.lib.bsa_set_state(self.h, n, *[ptr(a) for a in arrs]), 'bsa_set_state')
        self.n = n

    def set_intruder(self, lat=None, lon=None, trk=None, gs=None, alt=None, vs=None):
        self.gen += 1
        if lat is None:
            self.check(self.lib.bsa_set_intruder(self.h, 0, *([None] * 6)), 'bsa_set_intruder')
            return
        arrs = [f64(x) for x in (lat, lon, trk, gs, alt, vs)]
        self.check(self.lib.bsa_set_intruder(self.h, len(arrs[0]), *[ptr(a) for a in arrs]),
                   'bsa_set_intruder')

    # ---------------------------------------------------------------- detect
    def detect(self, rpz, hpz, tla, flags=0, row_begin=0, row_end=-1):
        self.gen += 1
        nc = ctypes.c_int64()
        nl = ctypes.c_int64()
        self.check(self.lib.bsa_detect(self.h, float(rpz), float(hpz), float(tla), int(flags),
                                       int(row_begin), int(row_end), ctypes.byref(nc),
                                       ctypes.byref(nl)), 'bsa_detect')
        self._rows = (row_begin, self.n if row_end is None or row_end < 0 else row_end)
        return nc.value, nl.value

    def fetch_pairs(self, n_conf, n_los, with_dcpa=False):
        P, L = n_conf, n_los
        R = self._rows[1] - self._rows[0]
        o = dict(ci=np.empty(P, np.int32), cj=np.empty(P, np.int32), qdr=np.empty(P),
                 dist=np.empty(P), tcpa=np.empty(P), tinconf=np.empty(P),
                 dcpa=np.empty(P) if with_dcpa else None, li=np.empty(L, np.int32),
                 lj=np.empty(L, np.int32), inconf=np.empty(R, np.uint8), tcpamax=np.empty(R))
        self.check(self.lib.bsa_fetch_pairs(
            self.h, ptr(o['ci'], _c_i32p), ptr(o['cj'], _c_i32p), ptr(o['qdr']), ptr(o['dist']),
            ptr(o['tcpa']), ptr(o['tinconf']), ptr(o['dcpa']), ptr(o['li'], _c_i32p),
            ptr(o['lj'], _c_i32p), ptr(o['inconf'], _c_u8p), ptr(o['tcpamax'])), 'bsa_fetch_pairs')
        return o

    ENVELOPE_FIELDS = ('hmax', 'vmin', 'vmax', 'vsmin', 'vsmax', 'axmax')

    def sim_set_limits(self, env=None):
        """OpenAP envelope for Pilot.applylimits in the resident step (bsa_sim_set_limits);
        ``env`` = dict of the six per-aircraft arrays, None switches the limits off."""
        if env is None:
            self.check(self.lib.bsa_sim_set_limits(self.h, *([None] * 6)), 'bsa_sim_set_limits')
            return
        arrs = [f64(env[k]).ravel() for k in self.ENVELOPE_FIELDS]
        self.check(self.lib.bsa_sim_set_limits(self.h, *[ptr(a) for a in arrs]), 'bsa_sim_set_limits')

    # ---------------------------------------------------------------- wind field
    def set_windfield(self, lat=None, lon=None, vnorth=None, veast=None):
        """2-D wind field for winddim 2 (bsa_set_windfield); no arguments clears it."""
        if lat is None:
            self.check(self.lib.bsa_set_windfield(self.h, 0, None, None, None, None), 'bsa_set_windfield')
            return
        arrs = [f64(x).ravel() for x in (lat, lon, vnorth, veast)]
        if len({len(a) for a in arrs}) != 1:
            raise ValueError('wind field arrays differ in length')
        self.check(self.lib.bsa_set_windfield(self.h, len(arrs[0]), *[ptr(a) for a in arrs]),
                   'bsa_set_windfield')

    def set_windfield3d(self, lat=None, lon=None, vnorth=None, veast=None, altstep=None):
        """3-D wind field for winddim 3 (bsa_set_windfield3d): Windfield.lat / lon of
        the nvec points, Windfield.vnorth / veast (nalt x nvec) and Windfield.altstep [m];
        no arguments clears it."""
        if lat is None:
            self.check(self.lib.bsa_set_windfield3d(self.h, 0, 0, 0.0, None, None, None, None),
                       'bsa_set_windfield3d')
            return
        pts = [f64(x).ravel() for x in (lat, lon)]
        tabs = [np.ascontiguousarray(x, dtype=np.float64) for x in (vnorth, veast)]
        nvec = len(pts[0])
        if len(pts[1]) != nvec or tabs[0].ndim != 2 or tabs[0].shape != tabs[1].shape or tabs[0].shape[1] != nvec:
            raise ValueError('3-D wind field: lat / lon of nvec points, vnorth / veast of shape (nalt, nvec)')
        if altstep is None:
            raise ValueError('3-D wind field: altstep [m] is required')
        self.check(self.lib.bsa_set_windfield3d(self.h, nvec, tabs[0].shape[0], float(altstep),
                                                *[ptr(a) for a in pts + tabs]), 'bsa_set_windfield3d')

    def wind_getdata(self, winddim, lat, lon, alt=None):
        """Windfield.getdata at the given positions (bsa_wind_getdata): winddim 1 / 2 from
        the 2-D field, 3 from the 3-D field at ``alt`` [m].  Returns (vnorth, veast)."""
        lat, lon = f64(lat).ravel(), f64(lon).ravel()
        n = len(lat)
        if len(lon) != n:
            raise ValueError('lat and lon differ in length')
        if alt is not None:
            alt = f64(alt).ravel()
            if len(alt) != n:
                raise ValueError('alt and lat differ in length')
        vn, ve = np.empty(n), np.empty(n)
        self.check(self.lib.bsa_wind_getdata(self.h, int(winddim), n, ptr(lat), ptr(lon),
                                             None if alt is None else ptr(alt), ptr(vn), ptr(ve)),
                   'bsa_wind_getdata')
        return vn, ve

    # ---------------------------------------------------------------- ACDATA feed
    def sim_acdata_request(self):
        self.check(self.lib.bsa_sim_acdata_request(self.h), 'bsa_sim_acdata_request')

    def sim_acdata_poll(self, wait=True):
        """The requested snapshot as a dict, or None while it is in flight (wait=False)."""
        probe = AcData()   # NULL arrays: status and row range only (no stream sync)
        st = self.lib.bsa_sim_acdata_poll(self.h, int(bool(wait)), ctypes.byref(probe))
        if st == 1:
            return None
        self.check(st, 'bsa_sim_acdata_poll')
        nr = probe.row_end - probe.row_begin
        arr = {k: np.empty(nr) for k in ACDATA_F64}
        arr.update(inconf=np.empty(nr, np.uint8), asasn=np.empty(nr, np.float32),
                   asase=np.empty(nr, np.float32))
        o = AcData(**{k: ptr(arr[k]) for k in ACDATA_F64}, inconf=ptr(arr['inconf'], _c_u8p),
                   asasn=ptr(arr['asasn'], _c_fp), asase=ptr(arr['asase'], _c_fp))
        self.check(self.lib.bsa_sim_acdata_poll(self.h, 1, ctypes.byref(o)), 'bsa_sim_acdata_poll')
        arr['inconf'] = arr['inconf'].astype(bool)
        arr.update({k: getattr(o, k) for k in ('steps', 'row_begin', 'row_end') + ACDATA_COUNTS})
        return arr

    # ---------------------------------------------------------------- geo matrices
    def qdrdist(self, lat1, lon1, lat2, lon2, kwik=False, pairwise=False):
        """bsa_qdrdist: (qdr, dist) as flat float64 arrays of m*n (outer) or m
        (pairwise) entries, row-major [i, j]."""
        la1, lo1, la2, lo2 = (f64(x).ravel() for x in (lat1, lon1, lat2, lon2))
        m, n = len(la1), len(la2)
        if len(lo1) != m or len(lo2) != n:
            raise ValueError('lat/lon lengths differ')
        total = m if pairwise else m * n
        qdr, dist = np.empty(total), np.empty(total)
        flags = (GEO_KWIK if kwik else 0) | (GEO_PAIRWISE if pairwise else 0)
        self.check(self.lib.bsa_qdrdist(self.h, m, ptr(la1), ptr(lo1), n, ptr(la2), ptr(lo2), flags,
                                        ptr(qdr), ptr(dist)), 'bsa_qdrdist')
        return qdr, dist

    def geo_last_ms(self):
        v = ctypes.c_double()
        self.check(self.lib.bsa_geo_last_ms(self.h, ctypes.byref(v)), 'bsa_geo_last_ms')
        return v.value

    def last_candidates(self):
        v = ctypes.c_int64()
        self.check(self.lib.bsa_last_candidates(self.h, ctypes.byref(v)), 'bsa_last_candidates')
        return v.value

    def set_candidate_capacity(self, capacity):
        """Candidate-list capacity for the next detects (grown on overflow)."""
        self.check(self.lib.bsa_set_candidate_capacity(self.h, int(capacity)),
                   'bsa_set_candidate_capacity')

    def set_candidate_reuse(self, on=True, sigma_h=800.0, sigma_v=60.0):
        """bsa_set_candidate_reuse: keep the candidate list across detects while
        every aircraft's drift stays inside its budgets (exact either way)."""
        self.check(self.lib.bsa_set_candidate_reuse(self.h, int(bool(on)), float(sigma_h), float(sigma_v)),
                   'bsa_set_candidate_reuse')

    def set_tile_reuse(self, on=True, sigma_h=2016.0, sigma_v=300.0):
        """bsa_set_tile_reuse: keep the resident detect's tile-pair list (K0d) while
        every prefilter record stays within the budgets of its build-time record."""
        self.check(self.lib.bsa_set_tile_reuse(self.h, int(bool(on)), float(sigma_h), float(sigma_v)),
                   'bsa_set_tile_reuse')

    def tile_reuse_stats(self):
        v = np.zeros(2, np.int64)
        self.check(self.lib.bsa_tile_reuse_stats(self.h, ptr(v, _c_i64p)), 'bsa_tile_reuse_stats')
        return dict(builds=int(v[0]), detects=int(v[1]))

    def set_hk(self, on=True, f=0.75):
        """Host-known tile-pair list decisions of the resident step (bsa_set_hk)."""
        self.check(self.lib.bsa_set_hk(self.h, 1 if on else 0, float(f)), 'bsa_set_hk')

    def set_halo_overlap(self, mode):
        """Halo exchange overlapped with the own tiles' sweep (bsa_set_halo_overlap):
        0 off, 1 several ranks, 2 also the one-GPU probe."""
        self.check(self.lib.bsa_set_halo_overlap(self.h, int(mode)), 'bsa_set_halo_overlap')

    def halo_overlap_count(self):
        v = np.zeros(1, np.int64)
        self.check(self.lib.bsa_halo_overlap_count(self.h, ptr(v, _c_i64p)), 'bsa_halo_overlap_count')
        return int(v[0])

    def hk_stats(self):
        v = np.zeros(6, np.int64)
        self.check(self.lib.bsa_hk_stats(self.h, ptr(v, _c_i64p)), 'bsa_hk_stats')
        return dict(keeps=int(v[0]), builds=int(v[1]), waits=int(v[2]), stale_aborts=int(v[3]),
                    cooldown=int(v[4]), on=bool(v[5]))

    def reuse_stats(self):
        b, d = ctypes.c_int64(), ctypes.c_int64()
        self.check(self.lib.bsa_reuse_stats(self.h, ctypes.byref(b), ctypes.byref(d)), 'bsa_reuse_stats')
        return dict(builds=b.value, detects=d.value)

    def reuse_budget_use(self):
        u = np.zeros(2)
        self.check(self.lib.bsa_reuse_budget_use(self.h, ptr(u)), 'bsa_reuse_budget_use')
        return float(u[0]), float(u[1])

    def last_tiles(self):
        kept, total, groups = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self.check(self.lib.bsa_last_tiles(self.h, ctypes.byref(kept), ctypes.byref(total),
                                           ctypes.byref(groups)), 'bsa_last_tiles')
        return kept.value, total.value, groups.value

    def last_timings(self):
        t = np.zeros(5)
        self.check(self.lib.bsa_last_timings(self.h, ptr(t)), 'bsa_last_timings')
        return dict(prep=t[0], prefilter=t[1], exact=t[2], sort=t[3], total=t[4])

    def set_timing_sample(self, every):
        """Time one detect in ``every`` (bsa_set_timing_sample; 0 = none)."""
        self.check(self.lib.bsa_set_timing_sample(self.h, int(every)), 'bsa_set_timing_sample')

    def timing_reset(self):
        """Forget recorded detect timings / statistics (bsa_timing_reset)."""
        self.check(self.lib.bsa_timing_reset(self.h), 'bsa_timing_reset')

    def timing_summary(self):
        """Mean stage times [ms] over the detects since the last reset and the
        summed statistics (bsa_timing_summary)."""
        t = np.zeros(5)
        st = np.zeros(4, np.int64)
        self.check(self.lib.bsa_timing_summary(self.h, ptr(t), ptr(st, _c_i64p)), 'bsa_timing_summary')
        return (dict(prep=t[0], prefilter=t[1], exact=t[2], sort=t[3], total=t[4]),
                dict(groups=int(st[0]), candidates=int(st[1]), tiles=int(st[2]), detects=int(st[3])))

    def sync(self):
        self.check(self.lib.bsa_sync(self.h), 'bsa_sync')

    # ---------------------------------------------------------------- MVP
    def set_pairs(self, ci, cj, qdr, dist, tcpa, tlos):
        """bsa_set_pairs: external confpairs (row-major) for bsa_mvp."""
        self.gen += 1
        ci = np.ascontiguousarray(ci, dtype=np.int32)
        cj = np.ascontiguousarray(cj, dtype=np.int32)
        arrs = [f64(x) for x in (qdr, dist, tcpa, tlos)]
        self.check(self.lib.bsa_set_pairs(self.h, len(ci), ptr(ci, _c_i32p), ptr(cj, _c_i32p),
                                          *[ptr(a) for a in arrs]), 'bsa_set_pairs')
        self._rows = (0, self.n)

    def mvp(self, params, gseast, gsnorth, selalt, apvs, asas_alt, noreso=None, resooff=None):
        """bsa_mvp on the last detect's pairs; ``asas_alt`` (detect rows) is
        updated in place.  Returns dict(trk, tas, vs, asase, asasn)."""
        rows = self._rows[1] - self._rows[0]
        ins = [f64(x) for x in (gseast, gsnorth, selalt, apvs)]
        if asas_alt.dtype != np.float64 or not asas_alt.flags.c_contiguous or len(asas_alt) != rows:
            raise ValueError('asas_alt must be a contiguous float64 array of the detect rows')
        nr = None if noreso is None else np.ascontiguousarray(noreso, dtype=np.uint8)
        ro = None if resooff is None else np.ascontiguousarray(resooff, dtype=np.uint8)
        o = dict(trk=np.empty(rows), tas=np.empty(rows), vs=np.empty(rows),
                 asase=np.empty(rows, np.float32), asasn=np.empty(rows, np.float32))
        self.check(self.lib.bsa_mvp(self.h, ctypes.byref(params), *[ptr(a) for a in ins],
                                    ptr(nr, _c_u8p), ptr(ro, _c_u8p), ptr(asas_alt), ptr(o['trk']),
                                    ptr(o['tas']), ptr(o['vs']), ptr(o['asase'], _c_fp),
                                    ptr(o['asasn'], _c_fp)), 'bsa_mvp')
        return o

    # ---------------------------------------------------------------- multi-GPU
    def comm_init(self, nranks, rank, uid):
        if len(uid) != UNIQUE_ID_BYTES:
            raise ValueError('unique id must be %d bytes' % UNIQUE_ID_BYTES)
        self.check(self.lib.bsa_comm_init(self.h, int(nranks), int(rank), uid), 'bsa_comm_init')
        self.comm_rank_world = (int(rank), int(nranks))

    def comm_init_group(self, group, rank):
        """Join an in-process Group as ``rank`` (call from this rank's thread)."""
        self.check(self.lib.bsa_comm_init_group(self.h, group.h, int(rank)), 'bsa_comm_init_group')
        self.comm_rank_world = (rank, group.nranks)
        self.gen += 1

    def comm_info(self):
        """The communicator as its transport reports it (bsa_comm_info): with
        RCCL, ranks / rank / device are ncclCommCount / ncclCommUserRank /
        ncclCommCuDevice."""
        v = (ctypes.c_int * 4)()
        self.check(self.lib.bsa_comm_info(self.h, v), 'bsa_comm_info')
        return dict(transport=('none', 'rccl', 'group')[v[0]], ranks=v[1], rank=v[2], device=v[3])

    def gather_pairs(self, root=0, with_dcpa=False):
        """C2: every rank's last detect gathered to ``root`` in rank order
        (collective; bsa_gather_counts + bsa_gather_pairs).  Returns the
        fetch_pairs-style dict on the root, None elsewhere."""
        tot = np.zeros(3, np.int64)
        self.check(self.lib.bsa_gather_counts(self.h, ptr(tot, _c_i64p)), 'bsa_gather_counts')
        P, L, R = (int(x) for x in tot)
        rank = getattr(self, 'comm_rank_world', (0, 1))[0]
        if rank != root:
            self.check(self.lib.bsa_gather_pairs(self.h, int(root), None), 'bsa_gather_pairs')
            return None
        o = dict(ci=np.empty(P, np.int32), cj=np.empty(P, np.int32), qdr=np.empty(P), dist=np.empty(P),
                 tcpa=np.empty(P), tinconf=np.empty(P), dcpa=np.empty(P) if with_dcpa else None,
                 li=np.empty(L, np.int32), lj=np.empty(L, np.int32), inconf=np.empty(R, np.uint8),
                 tcpamax=np.empty(R))
        po = PairsOut(**{k: ptr(v, _c_i32p if v.dtype == np.int32 else (_c_u8p if v.dtype == np.uint8 else _c_dp))
                         for k, v in o.items() if v is not None})
        self.check(self.lib.bsa_gather_pairs(self.h, int(root), ctypes.byref(po)), 'bsa_gather_pairs')
        return o

    def allreduce_max(self, values):
        v = np.array(values, dtype=np.float64, copy=True).ravel()
        self.check(self.lib.bsa_comm_allreduce_max(self.h, ptr(v), len(v)), 'bsa_comm_allreduce_max')
        return v

    def allreduce_sum(self, values):
        v = np.array(values, dtype=np.float64, copy=True).ravel()
        self.check(self.lib.bsa_comm_allreduce_sum(self.h, ptr(v), len(v)), 'bsa_comm_allreduce_sum')
        return v

    # ---------------------------------------------------------------- resident sim
    def sim_init(self, state, params):
        self.gen += 1
        n = len(state['lat'])
        keep = {k: f64(state[k]) for k in SIM_STATE_FIELDS}
        for k, a in keep.items():
            if len(a) != n:
                raise ValueError('sim state %s has length %d != %d' % (k, len(a), n))
        st = SimState(**{k: ptr(a) for k, a in keep.items()})
        self.check(self.lib.bsa_sim_init(self.h, n, ctypes.byref(st), ctypes.byref(params)),
                   'bsa_sim_init')
        self.n = n
        st = self.sim_stats()
        self._rows = (st['row_begin'], st['row_end'])   # fetch_pairs after steps: this rank's rows

    def sim_set_perf(self, table=None, type_idx=None):
        """bsa_sim_set_perf: OpenAP phase-dependent envelope + acceleration in the
        step (``table``/``type_idx`` from bluesky_amd.perf.type_table); None = off."""
        if table is None:
            self.check(self.lib.bsa_sim_set_perf(self.h, 0, None, None), 'bsa_sim_set_perf')
            return
        tab = np.ascontiguousarray(table, dtype=np.float64)
        idx = np.ascontiguousarray(type_idx, dtype=np.int32).ravel()
        if tab.ndim != 2 or tab.shape[1] != 24:
            raise ValueError('type table must be ntypes x 24')
        if len(idx) != self.n:
            raise ValueError('type index has length %d != %d' % (len(idx), self.n))
        self._perf_keep = (tab, idx)
        self.check(self.lib.bsa_sim_set_perf(self.h, tab.shape[0], ptr(tab), ptr(idx, _c_i32p)),
                   'bsa_sim_set_perf')

    def sim_read_perf(self):
        """(phase uint8, ax float64) of this rank's rows (full-n arrays, other rows 0)."""
        ph = np.zeros(self.n, np.uint8)
        ax = np.zeros(self.n)
        self.check(self.lib.bsa_sim_read_perf(self.h, ptr(ph, _c_u8p), ptr(ax)), 'bsa_sim_read_perf')
        return ph, ax

    @staticmethod
    def _force_table(ftable):
        ft = np.ascontiguousarray(ftable, dtype=np.float64)
        if ft.ndim != 2 or ft.shape[1] != 16:
            raise ValueError('force table must be ntypes x 16')
        return ft

    def openap_forces(self, table, ftable, type_idx, mass, tas, vs, alt, phase=None, bank=None):
        """bsa_openap_forces: dict of FORCE_OUTPUTS (float64 [n]) for host arrays."""
        tab = np.ascontiguousarray(table, dtype=np.float64)
        ft = self._force_table(ftable)
        if tab.ndim != 2 or tab.shape[1] != 24 or tab.shape[0] != ft.shape[0]:
            raise ValueError('type table must be ntypes x 24 with the force table\'s row count')
        idx = np.ascontiguousarray(type_idx, dtype=np.int32).ravel()
        n = len(idx)
        arrs = [f64(a).ravel() for a in (mass, tas, vs, alt)]
        ph = None if phase is None else np.ascontiguousarray(phase, dtype=np.uint8).ravel()
        for a in arrs + ([ph] if ph is not None else []):
            if len(a) != n:
                raise ValueError('forces input has length %d != %d' % (len(a), n))
        out = {k: np.zeros(n) for k in FORCE_OUTPUTS}
        if bank is not None:
            out['bank'] = np.array(bank, dtype=np.float64).ravel()
            if len(out['bank']) != n:
                raise ValueError('bank has length %d != %d' % (len(out['bank']), n))
        self.check(self.lib.bsa_openap_forces(self.h, n, tab.shape[0], ptr(tab), ptr(ft), ptr(idx, _c_i32p),
                                              ptr(ph, _c_u8p), *[ptr(a) for a in arrs],
                                              *[ptr(out[k]) for k in FORCE_OUTPUTS]), 'bsa_openap_forces')
        return out

    def fms_update(self, rows, rt_off, rt_n, state):
        """bsa_fms_update: one Autopilot.update call with a forced FMS tick.
        ``rows`` / ``rt_off`` / ``rt_n``: the route table (bluesky_amd.fms.route_table);
        ``state``: dict of FMS_TRAFFIC, FMS_REALS, FMS_FLAGS, FMS_TARGETS arrays and
        ``iactwp``.  Returns a new dict of FMS_REALS, FMS_FLAGS, FMS_TARGETS and
        ``iactwp`` after the call."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != ROUTE_COLS:
            raise ValueError('route table must be nrows x %d' % ROUTE_COLS)
        off = np.ascontiguousarray(rt_off, dtype=np.int32).ravel()
        cnt = np.ascontiguousarray(rt_n, dtype=np.int32).ravel()
        n = len(off)
        tr = [f64(state[k]).ravel() for k in FMS_TRAFFIC]
        out = {k: np.array(state[k], dtype=np.float64).ravel() for k in FMS_REALS + FMS_TARGETS}
        out.update({k: np.array(state[k]).astype(np.uint8).ravel() for k in FMS_FLAGS})
        out['iactwp'] = np.array(state['iactwp'], dtype=np.int32).ravel()
        for k, a in list(zip(FMS_TRAFFIC, tr)) + list(out.items()) + [('rt_n', cnt)]:
            if len(a) != n:
                raise ValueError('FMS array %s has length %d != %d' % (k, len(a), n))
        st = FmsState(**{k: ptr(out[k]) for k in FMS_REALS}, **{k: ptr(out[k], _c_u8p) for k in FMS_FLAGS})
        self.check(self.lib.bsa_fms_update(self.h, n, rows.shape[0], ptr(rows), ptr(off, _c_i32p), ptr(cnt, _c_i32p),
                                           ptr(out['iactwp'], _c_i32p), *[ptr(a) for a in tr], ctypes.byref(st),
                                           *[ptr(out[k]) for k in FMS_TARGETS]), 'bsa_fms_update')
        for k in FMS_FLAGS:
            out[k] = out[k].astype(bool)
        return out

    def fms_recover(self, rows, rt_off, rt_n, state, count):
        """bsa_fms_recover: Route.findact + Route.direct applied ``count[k]`` times to
        aircraft k.  ``rows`` / ``rt_off`` / ``rt_n`` / ``state`` as ``fms_update`` takes
        them (of FMS_TRAFFIC ``ax`` is not read and may be absent; of FMS_TARGETS only
        ``ap_alt``).  Returns a new dict of FMS_REALS, FMS_FLAGS, ``ap_alt`` and
        ``iactwp`` after the call."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != ROUTE_COLS:
            raise ValueError('route table must be nrows x %d' % ROUTE_COLS)
        off = np.ascontiguousarray(rt_off, dtype=np.int32).ravel()
        cnt = np.ascontiguousarray(rt_n, dtype=np.int32).ravel()
        count = np.ascontiguousarray(count, dtype=np.int32).ravel()
        n = len(off)
        names = [k for k in FMS_TRAFFIC if k != 'ax']
        tr = [f64(state[k]).ravel() for k in names]
        out = {k: np.array(state[k], dtype=np.float64).ravel() for k in FMS_REALS + ('ap_alt',)}
        out.update({k: np.array(state[k]).astype(np.uint8).ravel() for k in FMS_FLAGS})
        out['iactwp'] = np.array(state['iactwp'], dtype=np.int32).ravel()
        for k, a in list(zip(names, tr)) + list(out.items()) + [('rt_n', cnt), ('count', count)]:
            if len(a) != n:
                raise ValueError('FMS array %s has length %d != %d' % (k, len(a), n))
        st = FmsState(**{k: ptr(out[k]) for k in FMS_REALS}, **{k: ptr(out[k], _c_u8p) for k in FMS_FLAGS})
        self.check(self.lib.bsa_fms_recover(self.h, n, rows.shape[0], ptr(rows), ptr(off, _c_i32p), ptr(cnt, _c_i32p),
                                            ptr(out['iactwp'], _c_i32p), *[ptr(a) for a in tr], ctypes.byref(st),
                                            ptr(out['ap_alt']), ptr(count, _c_i32p)), 'bsa_fms_recover')
        for k in FMS_FLAGS:
            out[k] = out[k].astype(bool)
        return out

    def _route_check(self, rc, who):
        if rc > 0:
            raise RouteEditRefused(rc, '%s refused the batch (%s): %s' % (who, ROUTE_ERRORS.get(rc, rc),
                                                                             self.lib.bsa_last_error(self.h).decode()))
        self.check(rc, who)

    def route_edit(self, rows, rt_off, rt_n, state, records, wptype=None):
        """bsa_route_edit: a batch of route edit records (``route_records``) on host
        arrays.  ``rows`` / ``rt_off`` / ``rt_n`` / ``state`` as ``fms_recover`` takes them;
        ``wptype``: the waypoint type per row (None: all 0).  Returns ``(rows, rt_off,
        rt_n, wptype, state)``: the new table compacted in aircraft order and a new dict of
        FMS_REALS, FMS_FLAGS, ``ap_alt`` and ``iactwp``.  A refused batch raises
        RouteEditRefused."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, ROUTE_COLS)
        off = np.ascontiguousarray(rt_off, dtype=np.int32).ravel()
        cnt = np.ascontiguousarray(rt_n, dtype=np.int32).ravel()
        rec = route_records(records)
        n = len(off)
        wt = None if wptype is None else np.ascontiguousarray(wptype, dtype=np.uint8).ravel()
        if wt is not None and len(wt) != len(rows):
            raise ValueError('one waypoint type per table row')
        names = [k for k in FMS_TRAFFIC if k != 'ax']
        tr = [f64(state[k]).ravel() for k in names]
        out = {k: np.array(state[k], dtype=np.float64).ravel() for k in FMS_REALS + ('ap_alt',)}
        out.update({k: np.array(state[k]).astype(np.uint8).ravel() for k in FMS_FLAGS})
        out['iactwp'] = np.array(state['iactwp'], dtype=np.int32).ravel()
        for k, a in list(zip(names, tr)) + list(out.items()) + [('rt_n', cnt)]:
            if len(a) != n:
                raise ValueError('FMS array %s has length %d != %d' % (k, len(a), n))
        cap = len(rows) + len(rec)
        orows, otype = np.zeros((max(cap, 1), ROUTE_COLS)), np.zeros(max(cap, 1), np.uint8)
        ooff, ocnt, onrows = np.zeros(n, np.int32), np.zeros(n, np.int32), ctypes.c_int64()
        st = FmsState(**{k: ptr(out[k]) for k in FMS_REALS}, **{k: ptr(out[k], _c_u8p) for k in FMS_FLAGS})
        rc = self.lib.bsa_route_edit(self.h, n, rows.shape[0], ptr(rows), ptr(wt, _c_u8p), ptr(off, _c_i32p),
                                     ptr(cnt, _c_i32p), ptr(out['iactwp'], _c_i32p), *[ptr(a) for a in tr],
                                     ctypes.byref(st), ptr(out['ap_alt']), len(rec),
                                     rec.ctypes.data_as(_c_recp), cap, ptr(orows), ptr(otype, _c_u8p),
                                     ptr(ooff, _c_i32p), ptr(ocnt, _c_i32p), ctypes.byref(onrows))
        self._route_check(rc, 'bsa_route_edit')
        for k in FMS_FLAGS:
            out[k] = out[k].astype(bool)
        return orows[:onrows.value].copy(), ooff, ocnt, otype[:onrows.value].copy(), out

    def sim_route_edit(self, records):
        """bsa_sim_route_edit: the batch on the resident sim's table."""
        rec = route_records(records)
        self._route_check(self.lib.bsa_sim_route_edit(self.h, len(rec), rec.ctypes.data_as(_c_recp)), 'bsa_sim_route_edit')

    def sim_read_routes(self):
        """bsa_sim_read_routes: ``(rows, rt_off, rt_n, wptype)`` in aircraft order, compacted."""
        live = ctypes.c_int64()
        self._route_check(self.lib.bsa_sim_route_rows(self.h, ctypes.byref(live)), 'bsa_sim_route_rows')
        cap = max(int(live.value), 1)
        rows, wt = np.zeros((cap, ROUTE_COLS)), np.zeros(cap, np.uint8)
        off, cnt, got = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32), ctypes.c_int64()
        self._route_check(self.lib.bsa_sim_read_routes(self.h, cap, ptr(rows), ptr(wt, _c_u8p), ptr(off, _c_i32p),
                                                       ptr(cnt, _c_i32p), ctypes.byref(got)), 'bsa_sim_read_routes')
        return rows[:got.value].copy(), off, cnt, wt[:got.value].copy()

    def sim_route_stats(self):
        """bsa_sim_route_stats: dict of ``live``, ``dead``, ``written``, ``compactions``."""
        v = [ctypes.c_int64() for _ in range(4)]
        self._route_check(self.lib.bsa_sim_route_stats(self.h, *[ctypes.byref(x) for x in v]), 'bsa_sim_route_stats')
        return dict(zip(('live', 'dead', 'written', 'compactions'), (int(x.value) for x in v)))

    def sim_set_recovery(self, on=True):
        """bsa_sim_set_recovery: waypoint recovery after ResumeNav in the resident step."""
        self.check(self.lib.bsa_sim_set_recovery(self.h, 1 if on else 0), 'bsa_sim_set_recovery')

    # ---------------------------------------------------------------- turbulence
    def turb_draws(self, n, seed=0, call=0, first_index=0, raw=True):
        """bsa_turb_draws: (raw Philox words (n, 4) uint64 or None, unit normals (n, 3)) of the
        aircraft indices ``first_index .. first_index + n - 1`` of call number ``call``."""
        n = int(n)
        words = np.empty((n, 4), dtype=np.uint64) if raw else None
        z = np.empty((n, 3))
        self.check(self.lib.bsa_turb_draws(self.h, n, int(seed), int(call), int(first_index),
                                           ptr(words, _c_u64p), ptr(z)), 'bsa_turb_draws')
        return words, z

    def turb_apply(self, dt, sd, trk, coslat, lat, lon, alt, draws=None, seed=0, call=0):
        """bsa_turb_apply: one Turbulence.Woosh; ``draws``: the unit normals (hf, hw, alt) to
        apply, or None for the draws of (seed, call, index).  Returns the new (lat, lon, alt)."""
        sd = f64(sd).ravel()
        if len(sd) != 3:
            raise ValueError('sd: three standard deviations (flight direction, wing direction, vertical)')
        trk, coslat = f64(trk).ravel(), f64(coslat).ravel()
        out = [f64(x).ravel().copy() for x in (lat, lon, alt)]
        n = len(trk)
        z = [None] * 3 if draws is None else [f64(x).ravel() for x in draws]
        if any(len(x) != n for x in [coslat] + out + [x for x in z if x is not None]) or len(z) != 3:
            raise ValueError('turbulence arrays differ in length')
        self.check(self.lib.bsa_turb_apply(self.h, n, float(dt), ptr(sd), ptr(z[0]), ptr(z[1]), ptr(z[2]),
                                           int(seed), int(call), ptr(trk), ptr(coslat), *[ptr(x) for x in out]),
                   'bsa_turb_apply')
        return tuple(out)

    def sim_set_turbulence(self, on=True, sd=(0, 0.1, 0.1), seed=0):
        """bsa_sim_set_turbulence: Turbulence.Woosh as the last stage of every resident step."""
        sd = f64(sd).ravel()
        if len(sd) != 3:
            raise ValueError('sd: three standard deviations (flight direction, wing direction, vertical)')
        self.check(self.lib.bsa_sim_set_turbulence(self.h, 1 if on else 0, ptr(sd), int(seed)),
                   'bsa_sim_set_turbulence')

    def sim_turb_call(self, set_to=None):
        """bsa_sim_turb_call: the call number of the next step's draws (after setting it, if given)."""
        out = ctypes.c_int64(0)
        new = None if set_to is None else ctypes.byref(ctypes.c_int64(int(set_to)))
        self.check(self.lib.bsa_sim_turb_call(self.h, ctypes.byref(out), new), 'bsa_sim_turb_call')
        return out.value

    # ---------------------------------------------------------------- area filter
    def area_inside(self, areas, lat, lon, alt, nocull=False):
        """bsa_area_inside: ``areas`` as for ``area_table``.  Returns (inside (len(areas), n) bool,
        counts (len(areas),) uint64) from one launch."""
        lat, lon, alt = f64(lat).ravel(), f64(lon).ravel(), f64(alt).ravel()
        n, ns = len(lat), len(areas)
        if len(lon) != n or len(alt) != n:
            raise ValueError('area filter arrays differ in length')
        tab, verts = area_table(areas)
        W = (ns + 63) // 64
        words = np.zeros((W, n), dtype=np.uint64)
        counts = np.zeros(ns, dtype=np.uint64)
        self.check(self.lib.bsa_area_inside(self.h, n, ptr(lat), ptr(lon), ptr(alt), ns, tab, len(verts),
                                            ptr(verts), AREA_NOCULL if nocull else 0,
                                            ptr(words, _c_u64p), ptr(counts, _c_u64p)), 'bsa_area_inside')
        return area_unpack(words, ns), counts

    def sim_set_areas(self, areas):
        """bsa_sim_set_areas: the resident sim's area table (``areas`` as for ``area_table``; empty clears it)."""
        tab, verts = area_table(areas)
        self.check(self.lib.bsa_sim_set_areas(self.h, len(areas), tab, len(verts), ptr(verts)), 'bsa_sim_set_areas')

    def sim_set_sectors(self, shape_idx, every=1):
        """bsa_sim_set_sectors: sector k = shape ``shape_idx[k]`` of the table, a pass every ``every`` steps."""
        idx = np.ascontiguousarray(shape_idx, dtype=np.int32).ravel()
        self.check(self.lib.bsa_sim_set_sectors(self.h, len(idx), ptr(idx, _c_i32p), int(every)), 'bsa_sim_set_sectors')
        self._nsect = len(idx)

    def sim_sectors_poll(self, masks=False):
        """bsa_sim_sectors_poll: dict of count / arrived / left / arrived_total / left_total (per sector,
        uint64), step, updates; with ``masks`` also cur / prev (full-n uint64, this rank's rows filled)."""
        ns = getattr(self, '_nsect', 0)
        out = {k: np.zeros(ns, dtype=np.uint64) for k in ('count', 'arrived', 'left', 'arrived_total', 'left_total')}
        step, upd = ctypes.c_int64(0), ctypes.c_int64(0)
        cur = np.zeros(self.n, dtype=np.uint64) if masks else None
        prev = np.zeros(self.n, dtype=np.uint64) if masks else None
        self.check(self.lib.bsa_sim_sectors_poll(self.h, *[ptr(out[k], _c_u64p) for k in
                                                           ('count', 'arrived', 'left', 'arrived_total', 'left_total')],
                                                 ctypes.byref(step), ctypes.byref(upd), ptr(cur, _c_u64p),
                                                 ptr(prev, _c_u64p)), 'bsa_sim_sectors_poll')
        out.update(step=step.value, updates=upd.value)
        if masks:
            out.update(cur=cur, prev=prev)
        return out

    def sim_sectors_deleted(self):
        """bsa_sim_sectors_deleted: (positions in the last delete's index list, mask words) of this rank's
        deleted aircraft, read once."""
        cnt = ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_sectors_deleted(self.h, 0, None, None, ctypes.byref(cnt)), 'bsa_sim_sectors_deleted')
        pos, words = np.zeros(cnt.value, dtype=np.int64), np.zeros(cnt.value, dtype=np.uint64)
        if cnt.value:
            self.check(self.lib.bsa_sim_sectors_deleted(self.h, cnt.value, ptr(pos, _c_i64p), ptr(words, _c_u64p),
                                                        ctypes.byref(cnt)), 'bsa_sim_sectors_deleted')
        return pos, words

    # ---------------------------------------------------------------- geovectoring
    def geovec_apply(self, areas, rows, lat, lon, alt, trk, vs, selspd, ap_trk, selvs, selalt, nocull=False,
                     ngv=None):
        """bsa_geovec_apply: ``areas`` as for ``area_table``, ``rows`` as for ``geovec_rows`` (row k's
        ``shape`` indexes ``areas``).  Returns (dict of the four GEOVEC_TARGETS after the call, new
        arrays; changed (4,) uint64).  The inputs stay as they are."""
        tr = [f64(x).ravel() for x in (lat, lon, alt, trk, vs)]
        io = [np.array(f64(x).ravel()) for x in (selspd, ap_trk, selvs, selalt)]
        n = len(tr[0])
        if any(len(a) != n for a in tr + io):
            raise ValueError('geovector arrays differ in length')
        tab, verts = area_table(areas)
        gv, m = geovec_rows(rows)
        changed = np.zeros(4, dtype=np.uint64)
        self.check(self.lib.bsa_geovec_apply(self.h, n, *[ptr(a) for a in tr], len(areas), tab, len(verts), ptr(verts),
                                             m if ngv is None else int(ngv), gv, AREA_NOCULL if nocull else 0,
                                             *[ptr(a) for a in io], ptr(changed, _c_u64p)), 'bsa_geovec_apply')
        return dict(zip(GEOVEC_TARGETS, io)), changed

    def sim_set_geovectors(self, rows, every=1):
        """bsa_sim_set_geovectors: ``rows`` as for ``geovec_rows``, ``shape`` an index into the table of
        ``sim_set_areas``; applied every ``every`` steps; no rows = off."""
        gv, m = geovec_rows(rows)
        self.check(self.lib.bsa_sim_set_geovectors(self.h, m, gv, int(every)), 'bsa_sim_set_geovectors')

    def sim_geovec_stats(self):
        """bsa_sim_geovec_stats: dict of ``applies`` and ``changed`` (GEOVEC_TARGETS -> aircraft changed, this
        rank's rows, summed over the applications)."""
        applies = ctypes.c_int64(0)
        ch = np.zeros(4, dtype=np.uint64)
        self.check(self.lib.bsa_sim_geovec_stats(self.h, ctypes.byref(applies), ptr(ch, _c_u64p)), 'bsa_sim_geovec_stats')
        return dict(applies=applies.value, changed={k: int(v) for k, v in zip(GEOVEC_TARGETS, ch)})

    def sim_read_dropcount(self):
        """bsa_sim_read_dropcount: resopairs ResumeNav dropped per ownship in the last CD
        call (this rank's rows of a full-n int32 array, other rows 0)."""
        out = np.zeros(self.n, np.int32)
        self.check(self.lib.bsa_sim_read_dropcount(self.h, ptr(out, _c_i32p)), 'bsa_sim_read_dropcount')
        return out

    def sim_set_fms(self, rows=None, rt_off=None, rt_n=None, state=None, simt=0.0, t0=-999.):
        """bsa_sim_set_fms: Autopilot.update at the start of every resident step.
        ``rows`` / ``rt_off`` / ``rt_n`` / ``state`` as ``fms_update`` takes them (of
        ``state`` the FMS_REALS, FMS_FLAGS and ``iactwp``; the traffic and the targets
        are the sim's own); ``simt``: the time of the next step; None = off."""
        if rows is None:
            self.check(self.lib.bsa_sim_set_fms(self.h, 0, None, None, None, None, None, 0.0, 0.0), 'bsa_sim_set_fms')
            return
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != ROUTE_COLS:
            raise ValueError('route table must be nrows x %d' % ROUTE_COLS)
        pad = rows if len(rows) else np.zeros((1, ROUTE_COLS))        # (a table without rows is still "on")
        ints = [np.ascontiguousarray(a, dtype=np.int32).ravel() for a in (rt_off, rt_n, state['iactwp'])]
        keep = {k: f64(state[k]).ravel() for k in FMS_REALS}
        keep.update({k: np.ascontiguousarray(np.asarray(state[k]).astype(np.uint8)).ravel() for k in FMS_FLAGS})
        for k, a in list(keep.items()) + list(zip(('rt_off', 'rt_n', 'iactwp'), ints)):
            if len(a) != self.n:
                raise ValueError('FMS array %s has length %d != %d' % (k, len(a), self.n))
        st = FmsState(**{k: ptr(keep[k]) for k in FMS_REALS}, **{k: ptr(keep[k], _c_u8p) for k in FMS_FLAGS})
        self.check(self.lib.bsa_sim_set_fms(self.h, rows.shape[0], ptr(pad), *[ptr(a, _c_i32p) for a in ints],
                                            ctypes.byref(st), float(simt), float(t0)), 'bsa_sim_set_fms')

    def sim_read_fms(self):
        """dict of FMS_REALS, FMS_FLAGS (bool), ``iactwp``, FMS_TARGETS of this rank's
        rows (full-n arrays, other rows 0) and ``simt``, ``t0``, ``ticks``."""
        out = {k: np.zeros(self.n) for k in FMS_REALS + FMS_TARGETS}
        out.update({k: np.zeros(self.n, np.uint8) for k in FMS_FLAGS})
        out['iactwp'] = np.zeros(self.n, np.int32)
        st = FmsState(**{k: ptr(out[k]) for k in FMS_REALS}, **{k: ptr(out[k], _c_u8p) for k in FMS_FLAGS})
        simt, t0, ticks = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        self.check(self.lib.bsa_sim_read_fms(self.h, ctypes.byref(st), ptr(out['iactwp'], _c_i32p),
                                             *[ptr(out[k]) for k in FMS_TARGETS], ctypes.byref(simt),
                                             ctypes.byref(t0), ctypes.byref(ticks)), 'bsa_sim_read_fms')
        for k in FMS_FLAGS:
            out[k] = out[k].astype(bool)
        out.update(simt=simt.value, t0=t0.value, ticks=ticks.value)
        return out

    def sim_set_forces(self, ftable=None, mass=None):
        """bsa_sim_set_forces: OpenAP drag / thrust / fuel flow + fuel burnt in every
        step (``ftable`` / ``mass`` from bluesky_amd.perf.force_table); None = off."""
        if ftable is None:
            self.check(self.lib.bsa_sim_set_forces(self.h, 0, None, None), 'bsa_sim_set_forces')
            return
        ft = self._force_table(ftable)
        m = f64(mass).ravel()
        if len(m) != self.n:
            raise ValueError('mass has length %d != %d' % (len(m), self.n))
        self.check(self.lib.bsa_sim_set_forces(self.h, ft.shape[0], ptr(ft), ptr(m)), 'bsa_sim_set_forces')

    def sim_read_forces(self):
        """dict of FORCE_OUTPUTS + fuel_used of this rank's rows (full-n arrays, other rows 0)."""
        out = {k: np.zeros(self.n) for k in FORCE_OUTPUTS + ('fuel_used',)}
        self.check(self.lib.bsa_sim_read_forces(self.h, *[ptr(out[k]) for k in FORCE_OUTPUTS + ('fuel_used',)]),
                   'bsa_sim_read_forces')
        return out

    def sim_update(self, **arrays):
        """bsa_sim_update: overwrite the given full-n state arrays (SIM_STATE_FIELDS
        names) of the resident sim, keeping its ASAS bookkeeping."""
        bad = set(arrays) - set(SIM_STATE_FIELDS)
        if bad:
            raise ValueError('unknown sim state fields %s' % sorted(bad))
        keep = {k: f64(v) for k, v in arrays.items() if v is not None}
        for k, a in keep.items():
            if len(a) != self.n:
                raise ValueError('sim state %s has length %d != %d' % (k, len(a), self.n))
        st = SimState(**{k: ptr(a) for k, a in keep.items()})
        self.check(self.lib.bsa_sim_update(self.h, ctypes.byref(st)), 'bsa_sim_update')

    @staticmethod
    def _create_extra(extra, m):
        """(SimCreateExtra, the arrays it points into) for ``sim_create``'s ``extra``; ValueError for an unknown
        part, a wrong length or a dtype that would have to be truncated."""
        def arr(name, v, dtype, kinds):
            a = np.asarray(v)
            if a.dtype.kind not in kinds:
                raise ValueError('create: %s has dtype %s' % (name, a.dtype))
            a = np.ascontiguousarray(a, dtype=dtype).ravel()
            if len(a) != m:
                raise ValueError('create: %s has length %d != %d' % (name, len(a), m))
            return a
        bad = set(extra) - {'limits', 'type_idx', 'mass', 'fms'}
        if bad:
            raise ValueError('create: unknown parts %s' % sorted(bad))
        x, keep = SimCreateExtra(), {}
        if extra.get('limits') is not None:
            for k in Context.ENVELOPE_FIELDS:
                keep[k] = arr(k, extra['limits'][k], np.float64, 'fiu')
                setattr(x, k, ptr(keep[k]))
        if extra.get('type_idx') is not None:
            keep['type_idx'] = arr('type_idx', extra['type_idx'], np.int32, 'iu')
            x.type_idx = ptr(keep['type_idx'], _c_i32p)
        if extra.get('mass') is not None:
            keep['mass'] = arr('mass', extra['mass'], np.float64, 'fiu')
            x.mass = ptr(keep['mass'])
        if extra.get('fms') is not None:
            rows, off, cnt, state = extra['fms']
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            if rows.ndim != 2 or rows.shape[1] != ROUTE_COLS:
                raise ValueError('route table must be nrows x %d' % ROUTE_COLS)
            keep['rows'] = rows if len(rows) else np.zeros((1, ROUTE_COLS))   # (no rows is still a part)
            x.nrows, x.route_rows = rows.shape[0], ptr(keep['rows'])
            for k, v in (('rt_off', off), ('rt_n', cnt), ('iactwp', state['iactwp'])):
                keep[k] = arr(k, v, np.int32, 'iu')
                setattr(x, k, ptr(keep[k], _c_i32p))
            for k in FMS_REALS:
                keep[k] = arr(k, state[k], np.float64, 'fiu')
            for k in FMS_FLAGS:
                keep[k] = arr(k, state[k], np.uint8, 'biu')
            keep['st'] = FmsState(**{k: ptr(keep[k]) for k in FMS_REALS}, **{k: ptr(keep[k], _c_u8p) for k in FMS_FLAGS})
            x.st = ctypes.pointer(keep['st'])
        return x, keep

    def sim_create(self, state, extra=None):
        """bsa_sim_create: append aircraft (every SIM_STATE_FIELDS array, m long);
        they take indices n..n+m-1 (Traffic.create, traffic.py:192-312).  ``extra``
        (bsa_sim_create_with): dict of the parts of the stages that are on, m long each --
        ``limits`` (dict of ENVELOPE_FIELDS), ``type_idx``, ``mass``, ``fms`` = ``(rows, rt_off,
        rt_n, state)`` of the new aircraft alone, as ``sim_set_fms`` takes them for all."""
        m = len(state['lat'])
        keep = {k: f64(state[k]) for k in SIM_STATE_FIELDS}
        for k, a in keep.items():
            if len(a) != m:
                raise ValueError('created state %s has length %d != %d' % (k, len(a), m))
        st = SimState(**{k: ptr(a) for k, a in keep.items()})
        if extra is None:
            self.gen += 1
            self.check(self.lib.bsa_sim_create(self.h, m, ctypes.byref(st)), 'bsa_sim_create')
        else:
            x, parts = self._create_extra(extra, m)
            self.gen += 1
            self.check(self.lib.bsa_sim_create_with(self.h, m, ctypes.byref(st), ctypes.byref(x)), 'bsa_sim_create_with')
            if 'type_idx' in parts and getattr(self, '_perf_keep', None) is not None \
                    and len(self._perf_keep[1]) == self.n:                            # the host's copy follows
                self._perf_keep = (self._perf_keep[0], np.concatenate([self._perf_keep[1], parts['type_idx']]))
        self.n += m
        st = self.sim_stats()
        self._rows = (st['row_begin'], st['row_end'])

    def sim_delete(self, idx):
        """bsa_sim_delete: remove aircraft ``idx``; the rest shift down in order
        (Traffic.delete, traffic.py:364-378)."""
        d = np.unique(np.asarray(idx, dtype=np.int64).ravel())
        self.gen += 1
        self.check(self.lib.bsa_sim_delete(self.h, len(d), ptr(d, _c_i64p)), 'bsa_sim_delete')
        if getattr(self, '_perf_keep', None) is not None and len(self._perf_keep[1]) == self.n:
            self._perf_keep = (self._perf_keep[0], np.delete(self._perf_keep[1], d))
        self.n -= len(d)
        st = self.sim_stats()
        self._rows = (st['row_begin'], st['row_end'])

    def sim_step(self, nsteps=1):
        """bsa_sim_step; returns the steps run (fewer than ``nsteps`` when a condition fired)."""
        self.gen += 1
        self.check(self.lib.bsa_sim_step(self.h, int(nsteps)), 'bsa_sim_step')
        if not hasattr(self.lib, 'bsa_sim_steps_run'):   # (an older build loaded for an A/B measurement)
            return int(nsteps)
        return self.sim_steps_run()[0]

    def sim_steps_run(self):
        """bsa_sim_steps_run: (steps of the last sim_step call, the sim's step count)."""
        last, total = ctypes.c_int64(0), ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_steps_run(self.h, ctypes.byref(last), ctypes.byref(total)), 'bsa_sim_steps_run')
        return int(last.value), int(total.value)

    # ---------------------------------------------------------------- conditional commands
    @staticmethod
    def _cond_arrays(idx, condtype, target, lastdif):
        a = (np.ascontiguousarray(idx, dtype=np.int32).ravel(), np.ascontiguousarray(condtype, dtype=np.int32).ravel(),
             f64(target).ravel(), np.array(lastdif, dtype=np.float64).ravel())
        if any(len(x) != len(a[0]) for x in a):
            raise ValueError('condition arrays differ in length')
        return a

    def cond_update(self, idx, condtype, target, lastdif, alt, cas):
        """bsa_cond_update: one Condition.update; (fired condition indices ascending, new lastdif)."""
        idx, typ, target, last = self._cond_arrays(idx, condtype, target, lastdif)
        alt, cas = f64(alt), f64(cas)
        if len(alt) != len(cas):
            raise ValueError('alt and cas differ in length')
        m = len(idx)
        fired, count = np.zeros(max(m, 1), np.int32), ctypes.c_int64(0)
        self.check(self.lib.bsa_cond_update(self.h, m, ptr(idx, _c_i32p), ptr(typ, _c_i32p), ptr(target), ptr(last),
                                            len(alt), ptr(alt), ptr(cas), ptr(fired, _c_i32p), ctypes.byref(count)),
                   'bsa_cond_update')
        return fired[:count.value].astype(np.int64), last

    def sim_set_conditions(self, idx=(), condtype=(), target=(), lastdif=()):
        """bsa_sim_set_conditions: the table of the step's conditional commands (empty: off)."""
        idx, typ, target, last = self._cond_arrays(idx, condtype, target, lastdif)
        self.check(self.lib.bsa_sim_set_conditions(self.h, len(idx), ptr(idx, _c_i32p), ptr(typ, _c_i32p), ptr(target),
                                                   ptr(last)), 'bsa_sim_set_conditions')
        self._cond_cap = len(idx)

    def sim_cond_poll(self):
        """bsa_sim_cond_poll: (fired condition indices of the last stop, ascending; its step count)."""
        cap = max(getattr(self, '_cond_cap', 0), 1)
        fired, count, step = np.zeros(cap, np.int32), ctypes.c_int64(0), ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_cond_poll(self.h, cap, ptr(fired, _c_i32p), ctypes.byref(count), ctypes.byref(step)),
                   'bsa_sim_cond_poll')
        return fired[:count.value].astype(np.int64), int(step.value)

    def sim_read_conditions(self):
        """bsa_sim_read_conditions: dict of idx, condtype, target, lastdif of the live conditions."""
        cap = max(getattr(self, '_cond_cap', 0), 1)
        o = dict(idx=np.zeros(cap, np.int32), condtype=np.zeros(cap, np.int32), target=np.zeros(cap), lastdif=np.zeros(cap))
        count = ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_read_conditions(self.h, cap, ptr(o['idx'], _c_i32p), ptr(o['condtype'], _c_i32p),
                                                    ptr(o['target']), ptr(o['lastdif']), ctypes.byref(count)),
                   'bsa_sim_read_conditions')
        return {k: v[:count.value].copy() for k, v in o.items()}

    # ---------------------------------------------------------------- experiment area
    def exparea_update(self, gs, vs, alt, lat, lon, thrust, distance2D, distance3D, work, oldalt, inside, dt, area,
                       active=True, swtaxi=True, swtaxialt=1500 * 0.3048):
        """bsa_exparea_update: one Area.update (plugins/area.py:112-142).  ``area``: ``(type, coordinates,
        top, bottom)`` as for ``area_table``, or None (``name`` None: everything is outside).  Returns a dict
        of the updated distance2D / distance3D / work / oldalt / inside and delidx / delidxalt (ascending)."""
        ins = [f64(x).ravel() for x in (gs, vs, alt, lat, lon, thrust)]
        out = [f64(x).ravel().copy() for x in (distance2D, distance3D, work, oldalt)]
        flag = np.array(inside, dtype=bool).ravel().astype(np.uint8)
        n = len(ins[0])
        if any(len(x) != n for x in ins + out + [flag]):
            raise ValueError('experiment area arrays differ in length')
        tab, verts = (None, np.zeros((0, 2))) if area is None else area_table([area])
        l1, l2 = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        c1, c2 = ctypes.c_int64(0), ctypes.c_int64(0)
        self.check(self.lib.bsa_exparea_update(self.h, n, *[ptr(x) for x in ins + out], ptr(flag, _c_u8p), float(dt), tab,
                                               len(verts), ptr(verts), int(bool(active)), int(bool(swtaxi)),
                                               float(swtaxialt), ptr(l1, _c_i32p), ctypes.byref(c1), ptr(l2, _c_i32p),
                                               ctypes.byref(c2)), 'bsa_exparea_update')
        return dict(distance2D=out[0], distance3D=out[1], work=out[2], oldalt=out[3], inside=flag.astype(bool),
                    delidx=l1[:c1.value].astype(np.int64), delidxalt=l2[:c2.value].astype(np.int64))

    def sim_set_exparea(self, on, shape_idx=-1, dt=0.5, every=1, simt=0.0, active=True, swtaxi=True,
                        swtaxialt=1500 * 0.3048):
        """bsa_sim_set_exparea: the experiment area as the step's last stage (``shape_idx`` -1: no area)."""
        self.check(self.lib.bsa_sim_set_exparea(self.h, int(bool(on)), int(shape_idx), float(dt), int(every), float(simt),
                                                int(bool(active)), int(bool(swtaxi)), float(swtaxialt)),
                   'bsa_sim_set_exparea')

    def sim_exparea_simt(self, simt):
        """bsa_sim_exparea_simt: the sim time aircraft created from now on get as create_time."""
        self.check(self.lib.bsa_sim_exparea_simt(self.h, float(simt)), 'bsa_sim_exparea_simt')

    def sim_exparea_poll(self):
        """bsa_sim_exparea_poll: dict of delidx, delidxalt (ascending), step and ``records`` -- per exited
        aircraft a dict over EXPAREA_RECORD -- of the last stop; empty lists without one."""
        cap = max(self.n, 1)
        l1, l2 = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        rec = np.zeros((cap, len(EXPAREA_RECORD)))
        c1, c2, step = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_exparea_poll(self.h, cap, ptr(l1, _c_i32p), ctypes.byref(c1), ptr(l2, _c_i32p),
                                                 ctypes.byref(c2), ptr(rec), ctypes.byref(step)), 'bsa_sim_exparea_poll')
        r = rec[:c1.value]
        return dict(delidx=l1[:c1.value].astype(np.int64), delidxalt=l2[:c2.value].astype(np.int64), step=int(step.value),
                    records={k: r[:, q].copy() for q, k in enumerate(EXPAREA_RECORD)})

    def sim_read_exparea(self):
        """bsa_sim_read_exparea: dict of distance2D, distance3D, work, oldalt, create_time, inside (full n)."""
        keys = ('distance2D', 'distance3D', 'work', 'oldalt', 'create_time')
        o = {k: np.zeros(self.n) for k in keys}
        ins = np.zeros(self.n, np.uint8)
        self.check(self.lib.bsa_sim_read_exparea(self.h, *[ptr(o[k]) for k in keys], ptr(ins, _c_u8p)),
                   'bsa_sim_read_exparea')
        o['inside'] = ins.astype(bool)
        return o

    # ---------------------------------------------------------------- trails
    def trails_update(self, lat, lon, lastlat, lastlon, lasttim, t, dt, active=True, cap=None):
        """bsa_trails_update: one Trails.update(t) (traffic/trails.py:71-135).  Returns a dict of the updated
        lastlat / lastlon / lasttim and the segments lat0, lon0, lat1, lon1, time, idx in emission order.
        ``cap``: the room offered (default: n); more segments raise AccelError whose ``count`` is their number."""
        ins = [f64(x).ravel() for x in (lat, lon)]
        st = [f64(x).ravel().copy() for x in (lastlat, lastlon, lasttim)]
        n = len(ins[0])
        if any(len(x) != n for x in ins + st):
            raise ValueError('trail arrays differ in length')
        cap = n if cap is None else int(cap)
        seg = [np.zeros(max(cap, 1)) for _ in range(5)]
        idx, count = np.zeros(max(cap, 1), np.int32), ctypes.c_int64(-1)
        try:
            self.check(self.lib.bsa_trails_update(self.h, n, *[ptr(x) for x in ins + st], float(t), float(dt),
                                                  int(bool(active)), cap, *[ptr(x) for x in seg], ptr(idx, _c_i32p),
                                                  ctypes.byref(count)), 'bsa_trails_update')
        except AccelError as e:
            e.count = count.value
            raise
        m = count.value
        out = dict(lastlat=st[0], lastlon=st[1], lasttim=st[2], idx=idx[:m].astype(np.int64))
        out.update({k: v[:m].copy() for k, v in zip(('lat0', 'lon0', 'lat1', 'lon1', 'time'), seg)})
        return out

    def sim_set_trails(self, on, active=True, dt=10.0, simt=0.0, lasttim=0.0, max_segments=1 << 24):
        """bsa_sim_set_trails: Trails.update as a stage of every step.  ``lasttim``: a scalar or n values."""
        last = np.ascontiguousarray(np.broadcast_to(f64(lasttim), (self.n,))).copy() if on else None
        self.check(self.lib.bsa_sim_set_trails(self.h, int(bool(on)), int(bool(active)), float(dt), float(simt), ptr(last),
                                               int(max_segments)), 'bsa_sim_set_trails')

    def sim_trails_drain(self, last=True):
        """bsa_sim_trails_drain: dict of lat0, lon0, lat1, lon1, time, idx of the segments since the last drain, in
        emission order, and with ``last`` lastlat / lastlon by aircraft index."""
        cap = max(self.sim_read_trails(arrays=False)['undrained'], 1)
        ll = [np.zeros(self.n), np.zeros(self.n)] if last else [None, None]
        while True:
            seg = [np.zeros(cap) for _ in range(5)]
            idx, count = np.zeros(cap, np.int32), ctypes.c_int64(0)
            self.check(self.lib.bsa_sim_trails_drain(self.h, cap, *[ptr(x) for x in seg], ptr(idx, _c_i32p),
                                                     ctypes.byref(count), ptr(ll[0]), ptr(ll[1])), 'bsa_sim_trails_drain')
            if count.value <= cap:
                break
            cap = count.value
        m = count.value
        out = {k: v[:m].copy() for k, v in zip(('lat0', 'lon0', 'lat1', 'lon1', 'time'), seg)}
        out['idx'] = idx[:m].astype(np.int64)
        if last:
            out.update(lastlat=ll[0], lastlon=ll[1])
        return out

    def sim_read_trails(self, arrays=True):
        """bsa_sim_read_trails: dict of lastlat, lastlon, lasttim by aircraft index (with ``arrays``), ``simt`` (the
        t of the next step's update), ``last_t`` (the last step's) and ``undrained`` (segments on the device as of
        the last batch or drain)."""
        o = {k: np.zeros(self.n) for k in ('lastlat', 'lastlon', 'lasttim')} if arrays else {}
        simt, last_t, und = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_read_trails(self.h, *[ptr(o.get(k)) for k in ('lastlat', 'lastlon', 'lasttim')],
                                                ctypes.byref(simt), ctypes.byref(last_t), ctypes.byref(und)),
                   'bsa_sim_read_trails')
        o.update(simt=simt.value, last_t=last_t.value, undrained=int(und.value))
        return o

    # ---------------------------------------------------------------- ADS-B model
    @staticmethod
    def _adsb_mode(draws):
        if draws not in ADSB_DRAWS:
            raise ValueError("draws: 'shared' or 'per_aircraft'")
        return ADSB_DRAWS.index(draws)

    def adsb_draws(self, n, seed=0, call=0, first_index=0, stream=1, raw=True):
        """bsa_adsb_draws: (Philox words (n, 4) uint64 or None, unit normals (n, 3), uniforms (n,)) of the indices
        ``first_index .. first_index + n - 1`` of call ``call``; ``stream`` 1: the update's, 2: create's."""
        n = int(n)
        words = np.empty((n, 4), dtype=np.uint64) if raw else None
        z, u = np.empty((n, 3)), np.empty(n)
        self.check(self.lib.bsa_adsb_draws(self.h, n, int(seed), int(call), int(first_index), int(stream),
                                           ptr(words, _c_u64p), ptr(z), ptr(u)), 'bsa_adsb_draws')
        return words, z, u

    def adsb_update(self, time, traf, picture, trunctime=0.0, noise=False, transerror=(1e-4, 100 * 0.3048),
                    draws='shared', given=None, seed=0, call=0, first_index=0):
        """bsa_adsb_update: one ADSB.update(time).  ``traf``: dict of ADSB_FIELDS (the traffic's), ``picture``: dict
        of ``lastupdate`` and ADSB_FIELDS (the ADS-B object's).  ``given``: the unit normals to apply -- three values
        (shared) or (3, n) lat / lon / alt (per aircraft) -- or None for those of (seed, call, index).  Returns the
        new picture dict."""
        st = [f64(traf[k]).ravel() for k in ADSB_FIELDS]
        out = {k: f64(picture[k]).ravel().copy() for k in ('lastupdate',) + ADSB_FIELDS}
        n = len(st[0])
        if any(len(x) != n for x in st + list(out.values())):
            raise ValueError('ADS-B arrays differ in length')
        mode = self._adsb_mode(draws)
        te = f64(transerror).ravel()
        if len(te) != 2:
            raise ValueError('transerror: [lat / lon degrees, altitude metres]')
        z = None
        if given is not None:
            z = f64(given).ravel()
            if len(z) != (3 * n if mode else 3):
                raise ValueError('given draws: 3 values (shared) or 3 x n (per aircraft)')
        self.check(self.lib.bsa_adsb_update(self.h, n, float(time), float(trunctime), int(bool(noise)), ptr(te), mode,
                                            ptr(z), int(seed), int(call), int(first_index), *[ptr(x) for x in st],
                                            ptr(out['lastupdate']), *[ptr(out[k]) for k in ADSB_FIELDS]),
                   'bsa_adsb_update')
        return out

    def sim_set_adsb(self, on=True, noise=False, transerror=(1e-4, 100 * 0.3048), trunctime=0.0, seed=0,
                     draws='shared', simt=0.0, lastupdate=None):
        """bsa_sim_set_adsb: ADSB.update as a stage of every resident step.  ``lastupdate``: a scalar or n values
        (None: 0), read when the stage is switched on."""
        te = f64(transerror).ravel()
        if len(te) != 2:
            raise ValueError('transerror: [lat / lon degrees, altitude metres]')
        last = None
        if on:
            last = np.ascontiguousarray(np.broadcast_to(f64(0.0 if lastupdate is None else lastupdate), (self.n,))).copy()
        self.check(self.lib.bsa_sim_set_adsb(self.h, int(bool(on)), int(bool(noise)), ptr(te), float(trunctime), int(seed),
                                             self._adsb_mode(draws), float(simt), ptr(last)), 'bsa_sim_set_adsb')

    def sim_read_adsb(self):
        """bsa_sim_read_adsb: dict of ``lastupdate`` and ADSB_FIELDS of this rank's rows (full-n arrays, other rows 0),
        ``simt`` (the time of the next step's update) and ``call``."""
        o = {k: np.zeros(self.n) for k in ('lastupdate',) + ADSB_FIELDS}
        simt, call = ctypes.c_double(0.0), ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_read_adsb(self.h, *[ptr(o[k]) for k in ('lastupdate',) + ADSB_FIELDS],
                                              ctypes.byref(simt), ctypes.byref(call)), 'bsa_sim_read_adsb')
        o.update(simt=simt.value, call=int(call.value))
        return o

    def sim_adsb_call(self, set_to=None):
        """bsa_sim_adsb_call: the call number of the next noisy update (after setting it, if given)."""
        out = ctypes.c_int64(0)
        new = None if set_to is None else ctypes.byref(ctypes.c_int64(int(set_to)))
        self.check(self.lib.bsa_sim_adsb_call(self.h, ctypes.byref(out), new), 'bsa_sim_adsb_call')
        return out.value

    def sim_cd(self):
        """bsa_sim_cd: one CD call (detect -> resolver -> bookkeeping) without kinematics."""
        self.gen += 1
        self.check(self.lib.bsa_sim_cd(self.h), 'bsa_sim_cd')

    def sim_set_params(self, params):
        """bsa_sim_set_params: new rpz / hpz / tla / MVP switches for a running sim."""
        self.check(self.lib.bsa_sim_set_params(self.h, ctypes.byref(params)), 'bsa_sim_set_params')

    def sim_set_reso_lists(self, noreso=None, resooff=None):
        """bsa_sim_set_reso_lists: NORESO / RESOOFF membership (full-n bool-like arrays, None = empty)."""
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8).ravel() for a in (noreso, resooff)]
        for a in keep:
            if a is not None and len(a) != self.n:
                raise ValueError('membership array has length %d != %d' % (len(a), self.n))
        self.check(self.lib.bsa_sim_set_reso_lists(self.h, ptr(keep[0], _c_u8p), ptr(keep[1], _c_u8p)),
                   'bsa_sim_set_reso_lists')

    def sim_read_asas(self):
        """bsa_sim_read_asas: asas trk / tas / vs / alt, asase / asasn, active and the
        ResumeNav drops of this rank's rows (full-n arrays, other rows 0)."""
        n = self.n
        o = {k: np.zeros(n) for k in ('trk', 'tas', 'vs', 'alt')}
        o.update(asase=np.zeros(n, np.float32), asasn=np.zeros(n, np.float32), active=np.zeros(n, np.uint8),
                 dropped=np.zeros(n, np.uint8))
        ao = AsasOut(**{k: ptr(o[k]) for k in ('trk', 'tas', 'vs', 'alt')}, asase=ptr(o['asase'], _c_fp),
                     asasn=ptr(o['asasn'], _c_fp), active=ptr(o['active'], _c_u8p), dropped=ptr(o['dropped'], _c_u8p))
        self.check(self.lib.bsa_sim_read_asas(self.h, ctypes.byref(ao)), 'bsa_sim_read_asas')
        o['active'] = o['active'].astype(bool)
        o['dropped'] = o['dropped'].astype(bool)
        return o

    def sim_read(self):
        n = self.n
        o = {k: np.empty(n) for k in SIM_OUT_FIELDS}
        o['active'] = np.empty(n, np.uint8)
        so = SimOut(**{k: ptr(o[k]) for k in SIM_OUT_FIELDS}, active=ptr(o['active'], _c_u8p))
        self.check(self.lib.bsa_sim_read(self.h, ctypes.byref(so)), 'bsa_sim_read')
        o['active'] = o['active'].astype(bool)
        return o

    def sim_stats(self):
        v = np.zeros(6, np.int64)
        self.check(self.lib.bsa_sim_stats(self.h, ptr(v, _c_i64p)), 'bsa_sim_stats')
        return dict(steps=int(v[0]), cd_calls=int(v[1]), n_conf=int(v[2]), n_los=int(v[3]),
                    row_begin=int(v[4]), row_end=int(v[5]))

    def sim_aborts(self):
        """bsa_sim_aborts: batches aborted and re-run since sim_init."""
        out = ctypes.c_int64(0)
        self.check(self.lib.bsa_sim_aborts(self.h, ctypes.byref(out)), 'bsa_sim_aborts')
        return out.value

    def set_row_bucket(self, width):
        """bsa_set_row_bucket: K2's per-row bucket width (0 = scatter into segments)."""
        self.check(self.lib.bsa_set_row_bucket(self.h, int(width)), 'bsa_set_row_bucket')

    # ---------------------------------------------------------------- test seams (bsa_scan.hip)
    def scan_excl(self, x):
        """bsa_scan_excl: the device's exclusive prefix sum (mod 2^32) of the uint32 words ``x``."""
        x = np.ascontiguousarray(x, dtype=np.uint32).ravel()
        out = np.empty_like(x)
        self.check(self.lib.bsa_scan_excl(self.h, len(x), ptr(x, _c_u32p), ptr(out, _c_u32p)), 'bsa_scan_excl')
        return out

    def flagged_list(self, flag, id2h=None, mask=1, cap=None):
        """bsa_flagged_list: the indices i with ``flag[id2h[i]] & mask`` (``id2h`` None: ``flag[i]``),
        ascending.  ``cap``: the room offered (default: len(flag)); a longer list raises AccelError
        whose ``count`` is the list's true length."""
        flag = np.ascontiguousarray(flag, dtype=np.uint8).ravel()
        n = len(flag)
        if id2h is not None:
            id2h = np.ascontiguousarray(id2h, dtype=np.uint32).ravel()
            if len(id2h) != n:
                raise ValueError('flag and id2h differ in length')
        cap = n if cap is None else int(cap)
        out, count = np.zeros(max(cap, 1), np.int32), ctypes.c_int64(-1)
        try:
            self.check(self.lib.bsa_flagged_list(self.h, n, ptr(flag, _c_u8p), ptr(id2h, _c_u32p), int(mask), cap,
                                                 ptr(out, _c_i32p), ctypes.byref(count)), 'bsa_flagged_list')
        except AccelError as e:
            e.count = count.value
            raise
        return out[:count.value].astype(np.int64)

    def sim_row_ids(self):
        """Aircraft indices of this rank's rows, ascending (bsa_sim_row_ids): the
        rows of acdata / fetch_pairs' inconf and tcpamax after resident steps."""
        st = self.sim_stats()
        ids = np.empty(st['row_end'] - st['row_begin'], np.int32)
        self.check(self.lib.bsa_sim_row_ids(self.h, ptr(ids, _c_i32p)), 'bsa_sim_row_ids')
        return ids

    def sim_detect_rows(self, row_begin, row_end):
        """bsa_sim_detect_rows: the sim's detect of home rows [row_begin, row_end)
        (one rank's share, measured on one GPU); returns (n_conf, n_los)."""
        nc, nl = ctypes.c_int64(), ctypes.c_int64()
        self.check(self.lib.bsa_sim_detect_rows(self.h, int(row_begin), int(row_end), ctypes.byref(nc),
                                                ctypes.byref(nl)), 'bsa_sim_detect_rows')
        self.gen += 1
        self._rows = (int(row_begin), int(row_end))
        return nc.value, nl.value

    def sim_set_atmos(self, on=True):
        """bsa_sim_set_atmos: compute traf.p / rho / Temp = vatmos(alt) in every step."""
        self.check(self.lib.bsa_sim_set_atmos(self.h, int(bool(on))), 'bsa_sim_set_atmos')

    def sim_read_atmos(self):
        """(p, rho, Temp) of this rank's rows after the last step (full-n arrays)."""
        o = [np.zeros(self.n) for _ in range(3)]
        self.check(self.lib.bsa_sim_read_atmos(self.h, *[ptr(a) for a in o]), 'bsa_sim_read_atmos')
        return tuple(o)

    def sim_halo_stats(self):
        """bsa_sim_halo_stats: bytes received / sent per CD call, tiles received at the
        last CD call (or needed by the last bsa_sim_detect_rows share), regrowths."""
        v = np.zeros(4, np.int64)
        self.check(self.lib.bsa_sim_halo_stats(self.h, ptr(v, _c_i64p)), 'bsa_sim_halo_stats')
        return dict(rx_bytes=int(v[0]), tx_bytes=int(v[1]), tiles=int(v[2]), regrowths=int(v[3]))

    def sim_comm_stats(self):
        """bsa_sim_comm_stats: collectives since the last timing_reset (calls, bytes sent / received)."""
        v = np.zeros(3, np.int64)
        self.check(self.lib.bsa_sim_comm_stats(self.h, ptr(v, _c_i64p)), 'bsa_sim_comm_stats')
        return dict(calls=int(v[0]), tx_bytes=int(v[1]), rx_bytes=int(v[2]))

    def sim_set_halo_cap(self, sender, receiver, tiles):
        """bsa_sim_set_halo_cap (testing aid): this rank's copy of one tile capacity."""
        self.check(self.lib.bsa_sim_set_halo_cap(self.h, int(sender), int(receiver), int(tiles)),
                   'bsa_sim_set_halo_cap')

    def set_exact_fusion(self, on=True, max_records=64):
        """bsa_set_exact_fusion: K1b fused into the prefilter (default on); max_records < 64
        only to exercise the unfused retry in tests."""
        self.check(self.lib.bsa_set_exact_fusion(self.h, int(bool(on)), int(max_records)), 'bsa_set_exact_fusion')

    def exact_fusion_stats(self):
        """bsa_exact_fusion_stats: fused detects, their unfused retries, whether the last one fused."""
        v = np.zeros(3, np.int64)
        self.check(self.lib.bsa_exact_fusion_stats(self.h, ptr(v, _c_i64p)), 'bsa_exact_fusion_stats')
        return dict(fused=int(v[0]), retries=int(v[1]), last=bool(v[2]))

    def set_symmetric_sweep(self, on=True):
        """bsa_set_symmetric_sweep: each unordered tile pair swept once, refined both ways
        (default on where rows and columns are the same aircraft; results never depend on it)."""
        self.check(self.lib.bsa_set_symmetric_sweep(self.h, int(bool(on))), 'bsa_set_symmetric_sweep')

    def set_sweep_level(self, level=2):
        """bsa_set_symmetric_sweep by level: 0 both orders, 1 each unordered tile pair once,
        2 (a fresh context's) also the triangular sweep inside a diagonal tile pair."""
        self.check(self.lib.bsa_set_symmetric_sweep(self.h, int(level)), 'bsa_set_symmetric_sweep')

    def symmetric_sweep_stats(self):
        """bsa_symmetric_sweep_stats: detects planned symmetric, whether the last one was, its level."""
        v = np.zeros(2, np.int64)
        self.check(self.lib.bsa_symmetric_sweep_stats(self.h, ptr(v, _c_i64p)), 'bsa_symmetric_sweep_stats')
        return dict(detects=int(v[0]), last=bool(v[1]), level=int(v[1]))

    def set_lean_pairs(self, on=True):
        """bsa_set_lean_pairs: the CD steps of a step() call before its last skip the pair lists
        (default on; results never depend on it)."""
        self.check(self.lib.bsa_set_lean_pairs(self.h, int(on)), 'bsa_set_lean_pairs')   # (2: bsaccel.h, a testing aid)

    def lean_pairs_stats(self):
        """bsa_lean_pairs_stats: CD steps since the sim's init that ran lean / placed their pair lists."""
        v = np.zeros(2, np.int64)
        self.check(self.lib.bsa_lean_pairs_stats(self.h, ptr(v, _c_i64p)), 'bsa_lean_pairs_stats')
        return dict(lean=int(v[0]), full=int(v[1]))

    def listed_items(self, tier):
        """bsa_listed_items: the list slots of the items listed for the next detect, sorted."""
        n = np.zeros(1, np.int64)
        self.check(self.lib.bsa_listed_items(self.h, int(tier), None, 0, ptr(n, _c_i64p)), 'bsa_listed_items')
        out = np.zeros(max(int(n[0]), 1), np.uint32)
        self.check(self.lib.bsa_listed_items(self.h, int(tier), ptr(out, ctypes.POINTER(ctypes.c_uint32)), len(out),
                                             ptr(n, _c_i64p)), 'bsa_listed_items')
        return np.sort(out[:int(n[0])])

    def sim_probe_rank(self, rank, nranks):
        """bsa_sim_probe_rank (measurement aid): the one-rank sim's steps play rank `rank` of `nranks`."""
        self.check(self.lib.bsa_sim_probe_rank(self.h, int(rank), int(nranks)), 'bsa_sim_probe_rank')

    def sim_halo_recheck(self):
        """bsa_sim_halo_recheck (collective): the next exchange re-checks the region layout."""
        self.check(self.lib.bsa_sim_halo_recheck(self.h), 'bsa_sim_halo_recheck')

    def sim_asas_stats(self):
        """ASAS bookkeeping counts after the last CD call (resume_nav on); the
        unique / cumulative counts are None with several ranks."""
        v = np.zeros(6, np.int64)
        self.check(self.lib.bsa_sim_asas_stats(self.h, ptr(v, _c_i64p)), 'bsa_sim_asas_stats')
        opt = lambda x: None if x < 0 else int(x)
        return dict(resopairs=int(v[0]), confpairs_unique=opt(v[1]), lospairs_unique=opt(v[2]),
                    confpairs_all=opt(v[3]), lospairs_all=opt(v[4]), active=int(v[5]))

    def sim_resopairs(self):
        """This rank's resopairs as (idx1, idx2) int32 arrays, idx1-major; idx2 is
        -1 for an intruder deleted since the last CD call (bsa_sim_delete)."""
        cnt = np.zeros(1, np.int64)
        a = b = np.empty(0, np.int32)
        while True:
            self.check(self.lib.bsa_sim_resopairs(self.h, ptr(a, _c_i32p), ptr(b, _c_i32p), len(a),
                                                  ptr(cnt, _c_i64p)), 'bsa_sim_resopairs')
            if cnt[0] <= len(a):
                return a[:cnt[0]], b[:cnt[0]]
            a, b = np.empty(int(cnt[0]), np.int32), np.empty(int(cnt[0]), np.int32)

    # ---------------------------------------------------------------- kinematics
    KIN_OUT =('ax', 'delspd', 'cas', 'mach', 'gsnorth', 'gseast', 'gs', 'trk', 'coslat', 'az')

    def kinematics(self, simdt, state, inputs, winddim=0, windnorth=0.0, windeast=0.0):
        """bsa_kinematics.  ``state``: dict of float64 arrays tas, hdg, alt, vs,
        lat, lon (updated in place); ``inputs``: ptas, phdg, palt, pvs, bank,
        eps, accel.  Returns the output dict (incl. swhdgsel/swaltsel bool)."""
        n = len(state['tas'])
        io = KinIO()
        keep = []
        for k in ('ptas', 'phdg', 'palt', 'pvs', 'bank', 'eps', 'accel'):
            a = f64(inputs[k])
            keep.append(a)
            setattr(io, k, ptr(a))
        for k in ('tas', 'hdg', 'alt', 'vs', 'lat', 'lon'):
            a = state[k]
            if a.dtype != np.float64 or not a.flags.c_contiguous or len(a) != n:
                raise ValueError('state %s must be a contiguous float64 array' % k)
            setattr(io, k, ptr(a))
        out = {k: np.empty(n) for k in self.KIN_OUT}
        for k in self.KIN_OUT:
            setattr(io, k, ptr(out[k]))
        sw = {k: np.empty(n, np.uint8) for k in ('swhdgsel', 'swaltsel')}
        io.swhdgsel = ptr(sw['swhdgsel'], _c_u8p)
        io.swaltsel = ptr(sw['swaltsel'], _c_u8p)
        self.check(self.lib.bsa_kinematics(self.h, n, float(simdt), int(winddim), float(windnorth),
                                           float(windeast), ctypes.byref(io)), 'bsa_kinematics')
        out.update({k: v.astype(bool) for k, v in sw.items()})
        return out


_default = {}


def area_unpack(words, nshapes):
    """Mask words (W, n) uint64 -> inside (nshapes, n) bool: bit s % 64 of word s // 64."""
    words = np.asarray(words, dtype=np.uint64)
    s = np.arange(nshapes)
    if words.shape[0] == 0:
        return np.zeros((nshapes, words.shape[1]), dtype=bool)
    return ((words[s // 64] >> (s % 64).astype(np.uint64)[:, None]) & np.uint64(1)).astype(bool)


def default_context(device=0):
    """Process-wide lazily created context per device (like the sim's single bs.traf)."""
    ctx = _default.get(device)
    if ctx is None:
        ctx = _default[device] = Context(device)
    return ctx
