"""ctypes binding of libgaudi_hip.so (include/gaudi_hip.h).  There is NO CPU fallback: if the HIP
library is missing or a call fails, an exception is raised."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GAUDI_LIB", os.path.join(_PKG, "libgaudi_hip.so"))  # GAUDI_LIB: diagnostic builds


class GaudiError(RuntimeError):
    pass


class EdmConfig(C.Structure):
    _fields_ = [("in_node_nf", C.c_int32), ("hidden_nf", C.c_int32), ("n_layers", C.c_int32),
                ("inv_sublayers", C.c_int32), ("attention", C.c_int32), ("tanh", C.c_int32),
                ("coords_range", C.c_float), ("norm_constant", C.c_float), ("normalization_factor", C.c_float),
                ("diffusion_steps", C.c_int32), ("noise_power", C.c_float), ("noise_precision", C.c_float),
                ("norm_values", C.c_float * 3), ("sin_embedding", C.c_int32)]


class PredConfig(C.Structure):
    _fields_ = [("in_nf", C.c_int32), ("out_nf", C.c_int32), ("hidden_nf", C.c_int32), ("n_layers", C.c_int32),
                ("attention", C.c_int32), ("tanh", C.c_int32), ("coords_range", C.c_float)]


class Diag(C.Structure):
    _fields_ = [("max_masked_leak", C.c_float), ("max_cog_rel", C.c_float), ("max_cog_abs", C.c_float),
                ("nan_count", C.c_int32), ("reprojected", C.c_int32)]


class RingTables(C.Structure):
    _fields_ = [("n_types", C.c_int32), ("orientation", C.c_int32), ("check_dihedrals", C.c_int32), ("tol", C.c_double),
                ("min_dist", C.c_double), ("dist_lo", (C.c_double * 16) * 16), ("dist_hi", (C.c_double * 16) * 16),
                ("a3_count", C.c_int32 * 16), ("a3_lo", (C.c_double * 4) * 16), ("a3_hi", (C.c_double * 4) * 16),
                ("a4_0", C.c_double), ("a4_180", C.c_double)]


class StabilityAux(C.Structure):
    _fields_ = [("n_rings", C.c_int32), ("n_edges", C.c_int32), ("n_triplets", C.c_int32), ("n_nan_angles", C.c_int32),
                ("a3_min", C.c_float), ("a3_max", C.c_float), ("a4_min", C.c_float), ("a4_max", C.c_float)]


class AtomTables(C.Structure):
    """include/gaudi_hip.h: gaudi_atom_tables."""
    _fields_ = [("n_types", C.c_int32), ("ring_size", C.c_int32 * 16), ("ring_elem", (C.c_int32 * 6) * 16),
                ("templ", ((C.c_double * 2) * 6) * 16), ("no_orientation", C.c_int32 * 16), ("extra_angle", C.c_double * 16),
                ("n_template_h", C.c_int32 * 16), ("template_h_parent", (C.c_int32 * 2) * 16), ("h_elem", C.c_int32),
                ("c_elem", C.c_int32), ("h_bond", C.c_double)]


class PerceptionTables(C.Structure):
    """include/gaudi_hip.h: gaudi_perception_tables."""
    _fields_ = [("n_elems", C.c_int32), ("cov_radius", C.c_double * 8), ("h_elem", C.c_int32), ("c_elem", C.c_int32),
                ("b_elem", C.c_int32), ("n_types", C.c_int32), ("ring_size", C.c_int32 * 16), ("ring_elem", (C.c_int32 * 6) * 16),
                ("no_orientation", C.c_int32 * 16), ("db_type", C.c_int32), ("dhdb_type", C.c_int32)]


class ValenceTables(C.Structure):
    """include/gaudi_hip.h: gaudi_valence_tables."""
    _fields_ = [("n_elems", C.c_int32), ("n_options", (C.c_int32 * 5) * 8), ("option", (((C.c_int32 * 2) * 2) * 5) * 8),
                ("h_elem", C.c_int32), ("c_elem", C.c_int32)]


RINGS_MAX_ATOMS, RINGS_MAX_HEAVY, RINGS_MAX_RINGS = 384, 192, 32  # include/gaudi_hip.h: GAUDI_RINGS_MAX_*
RINGS_USE_H = 1
RINGS_OK, RINGS_NO_RINGS, RINGS_BAD_TYPE, RINGS_NOT_A_BASIS, RINGS_OVERFLOW = 0, 1, 2, 3, 4

ATOMS_MAX_ATOMS = 384  # include/gaudi_hip.h: GAUDI_ATOMS_MAX_ATOMS / GAUDI_ATOMS_MAX_BONDS
ATOMS_MAX_BONDS = 384
ATOMS_PLACE_H, ATOMS_FINGERPRINT = 1, 2

BONDS_MAX_ATOMS, BONDS_MAX_HEAVY, BONDS_MAX_BONDS, BONDS_MAX_CHARGED = 384, 192, 384, 4  # include/gaudi_hip.h: GAUDI_BONDS_*
# include/gaudi_hip.h: GAUDI_KEKULE_*
KEKULE_BUDGET, KEKULE_MAX_SEL, KEKULE_MAX_EDGES = 1 << 20, 128, 192
(KEKULE_OK, KEKULE_NO_KEKULE, KEKULE_NOT_NEUTRAL, KEKULE_NOT_CONNECTED, KEKULE_BAD_VALENCE, KEKULE_BAD_INPUT, KEKULE_OVERFLOW,
 KEKULE_EMPTY, KEKULE_UNDECIDED) = range(9)
(BONDS_OK, BONDS_NO_STRUCTURE, BONDS_CAPPED, BONDS_NOT_CONNECTED, BONDS_BAD_VALENCE, BONDS_BAD_INPUT, BONDS_OVERFLOW,
 BONDS_EMPTY, BONDS_GAVE_UP) = range(9)

FP_BINS = (256, 512, 1024)  # include/gaudi_hip.h: gaudi_circular_fingerprint
# include/gaudi_hip.h: GAUDI_CANON_*
CANON_MAX_ATOMS, CANON_MAX_HEAVY, CANON_MAX_BONDS, CANON_MAX_DEGREE, CANON_MAX_NODES, CANON_MAX_DEPTH = 384, 192, 384, 8, 4096, 16
CANON_OK, CANON_GAVE_UP, CANON_BAD_INPUT, CANON_OVERFLOW, CANON_EMPTY = range(5)
# include/gaudi_hip.h: GAUDI_SUB_*
SUB_MAX_QUERY, SUB_MAX_PATTERNS, SUB_MAX_STEPS, SUB_H_EXACT, SUB_CLOSED = 32, 64, 8192, 1, 2
SUB_OK, SUB_GAVE_UP, SUB_BAD_INPUT, SUB_OVERFLOW, SUB_EMPTY, SUB_BAD_PATTERN = range(6)
# include/gaudi_hip.h: GAUDI_HUCKEL_*
HUCKEL_MAX_PI, HUCKEL_MAX_CLASSES, HUCKEL_MAX_SWEEPS, HUCKEL_OPEN_SHELL, HUCKEL_DEGENERATE = 128, 16, 30, 1, 2
HUCKEL_OK, HUCKEL_NOT_CONVERGED, HUCKEL_BAD_INPUT, HUCKEL_OVERFLOW, HUCKEL_EMPTY, HUCKEL_NO_PI, HUCKEL_BAD_TABLE = range(7)


class HuckelTables(C.Structure):
    """gaudi_huckel_tables (include/gaudi_hip.h)."""
    _fields_ = [("n_elems", C.c_int32), ("h_elem", C.c_int32), ("c_elem", C.c_int32), ("n_classes", C.c_int32),
                ("site_class", (C.c_int32 * 5) * 8), ("h", C.c_float * 16), ("n_e", C.c_int32 * 16), ("k", C.c_float * 16),
                ("k_pair", (C.c_float * 16) * 16)]
# include/gaudi_hip.h: GAUDI_PPP_*
PPP_MAX_ITERATIONS, PPP_OPEN_SHELL, PPP_BAD_GEOMETRY, PPP_DEGENERATE, PPP_SCF_CAP, PPP_JACOBI_CAP = 64, 7, 8, 2, 4, 8
PPP_MATAGA_NISHIMOTO, PPP_OHNO = 0, 1
PPP_CIS_MAX_WINDOW, PPP_CIS_MAX_STATES = 8, 64
PPP_CIS_JACOBI_CAP, PPP_CIS_TRUNCATED, PPP_CIS_WINDOW_EDGE, PPP_CIS_TRIPLET_UNSTABLE = 16, 32, 64, 128
PPP_OPEN_TIE = 256
PPP_CIS_FLAGS = PPP_CIS_JACOBI_CAP | PPP_CIS_TRUNCATED | PPP_CIS_WINDOW_EDGE | PPP_CIS_TRIPLET_UNSTABLE
# include/gaudi_hip.h: GAUDI_RING_CURRENT_*
RING_CURRENT_MAX_RINGS, RING_CURRENT_MAX_SIZE, RING_CURRENT_SMALL_GAP, RING_CURRENT_RINGS_UNDEFINED = 32, 6, 9, 1
REACTIVITY_KINDS, REACTIVITY_MAX_SLICES, REACTIVITY_SWEEP_CAP, REACTIVITY_RINGS_TRUNCATED = 3, 16, 1, 2


class PPPTables(C.Structure):
    """gaudi_ppp_tables (include/gaudi_hip.h)."""
    _fields_ = [("n_elems", C.c_int32), ("h_elem", C.c_int32), ("c_elem", C.c_int32), ("n_classes", C.c_int32),
                ("site_class", (C.c_int32 * 5) * 8), ("I", C.c_float * 16), ("gamma", C.c_float * 16), ("z", C.c_int32 * 16),
                ("k", C.c_float * 16), ("beta0", C.c_float), ("beta_pair", (C.c_float * 16) * 16)]

FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
DP = C.POINTER(C.c_double)
U8P = C.POINTER(C.c_uint8)
U32P = C.POINTER(C.c_uint32)
I64P = C.POINTER(C.c_int64)


class TargetSpec(C.Structure):
    """include/gaudi_hip.h: gaudi_target_spec."""
    _fields_ = [("K", C.c_int32), ("w", FP), ("q", FP), ("c", FP), ("side", IP), ("scale", FP),
                ("w_per_mol", C.c_int32), ("q_per_mol", C.c_int32), ("c_per_mol", C.c_int32), ("side_per_mol", C.c_int32),
                ("scale_per_mol", C.c_int32), ("t_lo", C.c_int32), ("t_hi", C.c_int32)]


# gaudi_target_cb(user, B, K, pred, t, dT_dpred_out)
TARGET_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, FP, C.c_float, FP)
# gaudi_target_cbz(user, B, N, D, K, z_s, pred, t, dT_dpred_out, dT_dz_out)
TARGET_CBZ = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, FP, FP, C.c_float, FP, FP)

EXPORTS = {
    "gaudi_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "gaudi_destroy": (None, [C.c_void_p]),
    "gaudi_last_error": (C.c_char_p, [C.c_void_p]),
    "gaudi_load_edm": (C.c_int, [C.c_void_p, C.POINTER(EdmConfig), C.c_int, C.POINTER(C.c_char_p), C.POINTER(FP),
                                 C.POINTER(C.c_int64)]),
    "gaudi_load_predictor": (C.c_int, [C.c_void_p, C.POINTER(PredConfig), C.c_int, C.POINTER(C.c_char_p),
                                       C.POINTER(FP), C.POINTER(C.c_int64)]),
    "gaudi_get_gamma": (C.c_int, [C.c_void_p, FP]),
    "gaudi_get_step_coefficients": (C.c_int, [C.c_void_p, FP]),
    "gaudi_phi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, FP, FP, FP]),
    "gaudi_predictor_fwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, FP, FP, FP]),
    "gaudi_predictor_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, FP, FP, FP, FP, FP]),
    "gaudi_step": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, FP, FP, FP, FP, FP, C.c_float, FP]),
    "gaudi_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, FP, FP, FP, FP]),
    "gaudi_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, C.c_uint64, C.c_int64, FP, C.c_float, FP,
                               C.c_float, FP, FP, FP, C.POINTER(Diag)]),
    "gaudi_sample_cb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, C.c_uint64, C.c_int64, FP, C.c_float, TARGET_CB,
                                  C.c_void_p, C.c_float, FP, FP, FP, C.POINTER(Diag)]),
    "gaudi_sample_cbz": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, C.c_uint64, C.c_int64, FP, C.c_float, TARGET_CBZ,
                                   C.c_void_p, C.c_float, FP, FP, FP, C.POINTER(Diag)]),
    "gaudi_sample_chain": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, C.c_uint64, C.c_int64, FP, C.c_float, C.c_int, FP]),
    "gaudi_predict_noised": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, IP, FP, FP, C.c_uint64, C.c_int64, FP, FP, FP]),
    "gaudi_check_stability": (C.c_int, [C.c_void_p, C.POINTER(RingTables), C.c_int, C.c_int, FP, IP, IP,
                                        C.POINTER(C.c_uint8), FP, FP, C.POINTER(StabilityAux)]),
    "gaudi_stability_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_rings_to_atoms": (C.c_int, [C.c_void_p, C.POINTER(RingTables), C.POINTER(AtomTables), C.c_int, C.c_int, FP, IP, IP,
                                       C.c_int, C.c_int, C.c_int, IP, IP, DP, DP, IP, IP, IP, C.POINTER(C.c_uint64)]),
    "gaudi_atoms_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_atoms_to_rings": (C.c_int, [C.c_void_p, C.POINTER(PerceptionTables), C.c_int, C.c_int, DP, IP, IP, C.c_int, C.c_double,
                                       C.c_int, IP, IP, IP, IP, IP, DP, IP, DP, C.POINTER(C.c_uint8)]),
    "gaudi_rings_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_host_atoms_to_rings": (C.c_int, [C.POINTER(PerceptionTables), C.c_int, C.c_int, DP, IP, IP, C.c_int, C.c_double,
                                            C.c_int, IP, IP, IP, IP, IP, DP, IP, DP, C.POINTER(C.c_uint8)]),
    "gaudi_bond_orders": (C.c_int, [C.c_void_p, C.POINTER(ValenceTables), C.c_int, C.c_int, C.c_int, IP, IP, IP, IP,
                                    C.POINTER(C.c_uint8), C.POINTER(C.c_int8), IP, IP]),
    "gaudi_bonds_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_host_bond_orders": (C.c_int, [C.POINTER(ValenceTables), C.c_int, C.c_int, C.c_int, IP, IP, IP, IP,
                                         C.POINTER(C.c_uint8), C.POINTER(C.c_int8), IP, IP]),
    "gaudi_canonical_order": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, IP, IP, IP, IP,
                                        C.POINTER(C.c_uint8), IP, C.POINTER(C.c_uint16), IP, IP]),
    "gaudi_canon_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_host_canonical_order": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, IP, IP, IP, IP,
                                             C.POINTER(C.c_uint8), IP, C.POINTER(C.c_uint16), IP, IP]),
    "gaudi_circular_fingerprint": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, IP, IP, C.c_int,
                                             C.c_int, U8P, IP, IP]),
    "gaudi_host_circular_fingerprint": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, IP, IP, C.c_int,
                                                  C.c_int, U8P, IP, IP]),
    "gaudi_fp_library_set": (C.c_int, [C.c_void_p, C.c_int, C.c_int, U8P]),
    "gaudi_fp_nearest": (C.c_int, [C.c_void_p, C.c_int, C.c_int, U8P, C.c_int, U8P, C.c_int, IP, IP, IP]),
    "gaudi_fp_common": (C.c_int, [C.c_void_p, C.c_int, C.c_int, U8P, C.c_int, U8P, IP]),
    "gaudi_host_fp_nearest": (C.c_int, [C.c_int, C.c_int, U8P, C.c_int, U8P, C.c_int, IP, IP, IP]),
    "gaudi_fp_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_fp_neighbours": (C.c_int, [C.c_void_p, C.c_int, C.c_int, U8P, C.c_int, C.c_int, IP, C.c_int64, I64P, IP]),
    "gaudi_host_fp_neighbours": (C.c_int, [C.c_int, C.c_int, U8P, C.c_int, C.c_int, IP, C.c_int64, I64P, IP]),
    "gaudi_fp_cluster": (C.c_int, [C.c_void_p, C.c_int, C.c_int, U8P, C.c_int, C.c_int] + [IP] * 5),
    "gaudi_host_fp_cluster": (C.c_int, [C.c_int, C.c_int, U8P, C.c_int, C.c_int] + [IP] * 5),
    "gaudi_fp_pick_diverse": (C.c_int, [C.c_void_p, C.c_int, C.c_int, U8P, C.c_int, U8P] + [C.c_int] * 4 + [IP] * 7),
    "gaudi_host_fp_pick_diverse": (C.c_int, [C.c_int, C.c_int, U8P, C.c_int, U8P] + [C.c_int] * 4 + [IP] * 7),
    "gaudi_fp_select_stages_get": (C.c_int, [C.c_void_p, DP]),
    "gaudi_substructure_search": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [IP] * 4 + [C.c_int] * 3 + [IP] * 5 + [IP, IP, U8P, IP, IP]),
    "gaudi_host_substructure_search": (C.c_int, [C.c_int] * 6 + [IP] * 4 + [C.c_int] * 3 + [IP] * 5 + [IP, IP, U8P, IP, IP]),
    "gaudi_host_substructure_root_steps": (C.c_int, [C.c_int]),
    "gaudi_substructure_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_huckel": (C.c_int, [C.c_void_p, C.POINTER(HuckelTables)] + [C.c_int] * 3 + [IP] * 5 + [FP, U8P] + [IP] * 6 + [FP] * 6 + [C.POINTER(C.c_int8)]),
    "gaudi_host_huckel": (C.c_int, [C.POINTER(HuckelTables)] + [C.c_int] * 3 + [IP] * 5 + [FP, U8P] + [IP] * 6 + [FP] * 6 + [C.POINTER(C.c_int8)]),
    "gaudi_huckel_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_ppp": (C.c_int, [C.c_void_p, C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, C.c_int, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6),
    "gaudi_host_ppp": (C.c_int, [C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, C.c_int, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6),
    "gaudi_ppp_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_ppp_open": (C.c_int, [C.c_void_p, C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, IP, C.c_int, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6 + [FP, C.POINTER(C.c_double), C.POINTER(C.c_double), IP, IP]),
    "gaudi_host_ppp_open": (C.c_int, [C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, IP, C.c_int, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6 + [FP, C.POINTER(C.c_double), C.POINTER(C.c_double), IP, IP]),
    "gaudi_ppp_open_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_ppp_scf": (C.c_int, [C.c_void_p, C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, IP, C.c_int, C.c_int32, C.c_int32, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6 + [FP, C.POINTER(C.c_double), C.POINTER(C.c_double), IP, IP, FP, IP]),
    "gaudi_host_ppp_scf": (C.c_int, [C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, IP, C.c_int, C.c_int32, C.c_int32, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6 + [FP, C.POINTER(C.c_double), C.POINTER(C.c_double), IP, IP, FP, IP]),
    "gaudi_ppp_scf_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_ppp_cis": (C.c_int, [C.c_void_p, C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, C.c_int, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6 + [C.c_int] + [FP] * 4 + [U8P, FP] + [IP] * 4),
    "gaudi_host_ppp_cis": (C.c_int, [C.POINTER(PPPTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP, C.c_int, C.c_float] + [FP, U8P, FP, FP, C.POINTER(C.c_int8)] + [IP] * 7 + [FP] * 6 + [C.c_int] + [FP] * 4 + [U8P, FP] + [IP] * 4),
    "gaudi_ppp_cis_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_kekule": (C.c_int, [C.c_void_p, C.POINTER(ValenceTables)] + [C.c_int] * 3 + [IP] * 4 + [I64P, U32P, IP, IP, U32P, IP, IP, I64P, IP]),
    "gaudi_host_kekule": (C.c_int, [C.POINTER(ValenceTables)] + [C.c_int] * 3 + [IP] * 4 + [I64P, U32P, IP, IP, U32P, IP, IP, I64P, IP]),
    "gaudi_kekule_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_ring_currents": (C.c_int, [C.c_void_p, C.POINTER(HuckelTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP] + [FP, IP, IP, IP] + [FP] * 6 + [IP] * 5),
    "gaudi_host_ring_currents": (C.c_int, [C.POINTER(HuckelTables)] + [C.c_int] * 3 + [IP] * 4 + [FP, IP] + [FP, IP, IP, IP] + [FP] * 6 + [IP] * 5),
    "gaudi_ring_currents_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_reactivity": (C.c_int, [C.c_void_p, C.POINTER(HuckelTables)] + [C.c_int] * 3 + [IP] * 5 + [C.c_int] * 2 + [FP, FP, IP, IP, FP, FP, FP] + [IP] * 6),
    "gaudi_host_reactivity": (C.c_int, [C.POINTER(HuckelTables)] + [C.c_int] * 3 + [IP] * 5 + [C.c_int] * 2 + [FP, FP, IP, IP, FP, FP, FP] + [IP] * 6),
    "gaudi_reactivity_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gaudi_philox_normal": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, FP]),
    "gaudi_host_schedule": (C.c_int, [C.c_int, C.c_float, C.c_float, FP, FP]),
    "gaudi_host_eigh3": (C.c_int, [C.c_int, DP, DP]),
    "gaudi_host_graph_meta": (C.c_int, [C.c_int, C.c_int, FP, FP, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), FP, C.c_int32,
                                        C.POINTER(C.c_int32)]),
    "gaudi_host_pack_matrix": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, FP, FP]),
    "gaudi_host_pack_matrix_split": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, FP, FP]),
    "gaudi_host_pack_matrix_f16": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, FP, FP]),
    "gaudi_host_weight_scale": (C.c_int, [C.c_int, C.POINTER(FP), IP, IP, IP, FP]),
    "gaudi_host_node_operand_offset": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP]),
    "gaudi_profile_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "gaudi_profile_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "gaudi_set_steps_per_launch": (C.c_int, [C.c_void_p, C.c_int]),
    "gaudi_set_readout_nodes": (C.c_int, [C.c_void_p, C.c_int]),
    "gaudi_set_fix_noise": (C.c_int, [C.c_void_p, C.c_int, C.c_int64]),
    "gaudi_host_graph_meta8": (C.c_int, [C.c_int, C.c_int, FP, FP, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), FP,
                                         C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.c_int32, C.POINTER(C.c_int32)]),
    "gaudi_kernel_variant": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gaudi_edge_math": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gaudi_node_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "gaudi_last_workgroups": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gaudi_host_pack_plan_wide": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, FP, FP, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gaudi_set_plan_hint": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "gaudi_last_warning": (C.c_char_p, [C.c_void_p]),
    "gaudi_last_kernel_key": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "gaudi_kernel_key_log": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "gaudi_host_kernel_keys": (C.c_int, [C.c_char_p, C.c_int]),
    "gaudi_abi_version": (C.c_int, []),
    "gaudi_last_family_split": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "gaudi_profile_clock": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "gaudi_last_keep_h": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "gaudi_host_pack_plan": (C.c_int, [C.c_int, C.c_int, FP, FP, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32)]),
    "gaudi_edm_nll": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, IP, FP, FP, C.c_uint64, C.c_int64, FP, FP, FP]),
    "gaudi_host_nll_terms": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, FP, FP, FP,
                                       IP, FP]),
    "gaudi_predictor_loss_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, IP, FP, FP, FP, C.c_uint64, C.c_int64, FP, FP,
                                            FP, FP, IP]),
    "gaudi_predictor_grad_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "gaudi_host_pred_train_layout": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(FP), C.POINTER(C.c_int64),
                                               IP, IP, FP]),
    "gaudi_edm_loss_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, IP, FP, FP, C.c_uint64, C.c_int64, FP, C.c_int, FP,
                                      FP, FP, FP, IP]),
    "gaudi_edm_grad_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "gaudi_edm_set_train_weights": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(FP), C.POINTER(C.c_int64)]),
    "gaudi_host_edm_train_layout": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(FP), C.POINTER(C.c_int64),
                                              IP, IP, FP]),
    "gaudi_host_train_floats_per_mol": (C.c_int, [C.c_int] * 8 + [C.POINTER(C.c_int64)]),
    "gaudi_host_edm_seed_coef": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, FP, FP, FP]),
    "gaudi_sample_grid": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, C.c_uint64, C.c_int64, FP, C.c_float, FP, C.c_float,
                                    C.c_int, IP, FP, FP, FP, FP, FP, FP, C.POINTER(Diag)]),
    "gaudi_step_pair": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, FP, FP, FP, FP, FP, C.c_float, FP]),
    "gaudi_sample_cb_grid": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, C.c_uint64, C.c_int64, FP, C.c_float, TARGET_CB,
                                       TARGET_CBZ, C.c_void_p, C.c_float, C.c_int, IP, FP, FP, FP, FP, FP, FP, C.POINTER(Diag)]),
    "gaudi_host_grid_coefficients": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_int, IP, FP, IP]),
    "gaudi_sample_target": (C.c_int, [C.c_void_p, C.c_int, C.c_int, FP, FP, C.c_uint64, C.c_int64, FP, C.c_float,
                                      C.POINTER(TargetSpec), C.c_int, IP, FP, FP, FP, FP, FP, FP, FP, C.POINTER(Diag)]),
    "gaudi_step_target": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, FP, FP, FP, FP, C.POINTER(TargetSpec), FP, FP]),
    "gaudi_host_target_seed": (C.c_int, [C.POINTER(TargetSpec), C.c_int, C.c_int, FP, FP]),
}

ABI_VERSION = 7  # include/gaudi_hip.h: GAUDI_ABI_VERSION
_ROUND6_EXPORTS = ("gaudi_last_warning", "gaudi_abi_version", "gaudi_last_family_split", "gaudi_profile_clock", "gaudi_last_keep_h")  # an older A/B library (GAUDI_LIB) lacks them
_NLL_EXPORTS = ("gaudi_edm_nll", "gaudi_predictor_loss_grad", "gaudi_predictor_grad_size", "gaudi_edm_loss_grad",
                "gaudi_edm_grad_size", "gaudi_edm_set_train_weights")  # ... and the NLL / training entry
# points (same ABI version: no existing signature changed)
_GRID_EXPORTS = ("gaudi_sample_grid", "gaudi_step_pair", "gaudi_sample_cb_grid")  # ... and the time-grid chains
_TARGET_EXPORTS = ("gaudi_sample_target", "gaudi_step_target")  # ... and the fused value targets
_ATOMS_EXPORTS = ("gaudi_rings_to_atoms", "gaudi_atoms_profile_get")  # ... and the graph-of-atoms conversion
_RINGS_EXPORTS = ("gaudi_atoms_to_rings", "gaudi_rings_profile_get")  # ... and the way back, atoms -> graph of rings
_BONDS_EXPORTS = ("gaudi_bond_orders", "gaudi_bonds_profile_get")  # ... and bond orders / formal charges
_CANON_EXPORTS = ("gaudi_canonical_order", "gaudi_canon_profile_get")  # ... and the canonical numbering
_FP_EXPORTS = ("gaudi_circular_fingerprint", "gaudi_fp_library_set", "gaudi_fp_nearest", "gaudi_fp_common",
               "gaudi_fp_profile_get", "gaudi_fp_neighbours", "gaudi_fp_cluster",
               "gaudi_fp_pick_diverse", "gaudi_fp_select_stages_get")  # ... and the circular fingerprints with their similarity, clusters and diverse picks
_SUB_EXPORTS = ("gaudi_substructure_search", "gaudi_substructure_profile_get")  # ... and the substructure search
_HUCKEL_EXPORTS = ("gaudi_huckel", "gaudi_huckel_profile_get")  # ... and the Hueckel levels
_PPP_EXPORTS = ("gaudi_ppp", "gaudi_ppp_profile_get", "gaudi_ppp_cis", "gaudi_ppp_cis_profile_get", "gaudi_ppp_open",
                "gaudi_ppp_open_profile_get", "gaudi_ppp_scf", "gaudi_ppp_scf_profile_get")  # ... and the PPP levels and excited states
_KEKULE_EXPORTS = ("gaudi_kekule", "gaudi_kekule_profile_get")  # ... and the Kekule structure counts
_RING_CURRENT_EXPORTS = ("gaudi_ring_currents", "gaudi_ring_currents_profile_get")  # ... and the ring currents
_REACTIVITY_EXPORTS = ("gaudi_reactivity", "gaudi_reactivity_profile_get")  # ... and the localization energies
_KEY_EXPORTS = ("gaudi_last_kernel_key", "gaudi_kernel_key_log", "gaudi_host_kernel_keys")  # ... and the names of the kernels launched / registered

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree library and bind every symbol of include/gaudi_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GaudiError(f"{LIB_PATH} not found: build it with `python -m gaudi_amd.build` "
                         "(there is no CPU fallback for the sampler)")
    lib = C.CDLL(LIB_PATH)
    # the host-side packers (gaudi_host_*) are test / tooling entry points: a diagnostic library named by GAUDI_LIB (an A/B
    # build of another revision) may predate some of them; everything else must be there
    lenient = "GAUDI_LIB" in os.environ
    # ... and one whose exported signatures differ (include/gaudi_hip.h: GAUDI_ABI_VERSION) must not have this file's argument
    # types bound to its host-side entry points at all: round 5 inserted a float into gaudi_host_pack_matrix_split, and a
    # call through the wrong prototype passes that float where the old library expects a pointer
    abi = None
    if hasattr(lib, "gaudi_abi_version"):
        lib.gaudi_abi_version.restype, lib.gaudi_abi_version.argtypes = C.c_int, []
        abi = int(lib.gaudi_abi_version())
    if abi != ABI_VERSION and not lenient:
        raise GaudiError(f"{LIB_PATH} exports ABI version {abi}, this package expects {ABI_VERSION}: rebuild it "
                         "(`python -m gaudi_amd.build --force`)")
    for name, (res, args) in EXPORTS.items():
        if lenient and not hasattr(lib, name) and (name.startswith("gaudi_host_") or name in _ROUND6_EXPORTS + _NLL_EXPORTS + _GRID_EXPORTS + _TARGET_EXPORTS + _ATOMS_EXPORTS + _RINGS_EXPORTS + _BONDS_EXPORTS + _CANON_EXPORTS + _FP_EXPORTS + _SUB_EXPORTS + _HUCKEL_EXPORTS + _PPP_EXPORTS + _KEKULE_EXPORTS + _RING_CURRENT_EXPORTS + _REACTIVITY_EXPORTS + _KEY_EXPORTS):
            continue
        if lenient and abi != ABI_VERSION and name.startswith("gaudi_host_"):
            continue  # left unbound on purpose: a call raises instead of corrupting memory
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def key_lines(fn, *head) -> list:
    """The lines of a key list (gaudi_host_kernel_keys / gaudi_kernel_key_log: a call with no buffer sizes it)."""
    need = fn(*head, None, 0)
    if need < 0:
        raise GaudiError(f"{fn.__name__} failed ({need})")
    buf = C.create_string_buffer(need)
    fn(*head, buf, need)
    return buf.value.decode().splitlines()


def registered_kernel_keys() -> list:
    """The key of every entry of the kernel table (csrc/kernel_table.h), sorted.  Needs no device."""
    return key_lines(load_library().gaudi_host_kernel_keys)


def rings_outputs(B: int, max_rings: int) -> dict:
    """The nine output arrays of gaudi_atoms_to_rings / gaudi_host_atoms_to_rings, in argument order."""
    M = int(max_rings)
    return dict(status=np.zeros(B, np.int32), n_rings=np.zeros(B, np.int32), ring_size=np.zeros((B, M), np.int32),
                ring_atoms=np.full((B, M, 6), -1, np.int32), ring_type=np.zeros((B, M), np.int32),
                centre=np.zeros((B, M, 3), np.float64), n_orient=np.zeros((B, M), np.int32),
                orient=np.zeros((B, M, 2, 3), np.float64), adj=np.zeros((B, M, M), np.uint8))


def rings_args(xyz, elem, n_atoms, flags, covalency_factor, max_rings, out):
    """The arguments both entry points share after the tables."""
    assert xyz.dtype == np.float64 and elem.dtype == np.int32 and n_atoms.dtype == np.int32
    assert xyz.flags["C_CONTIGUOUS"] and elem.flags["C_CONTIGUOUS"] and n_atoms.flags["C_CONTIGUOUS"]
    B, A = xyz.shape[0], xyz.shape[1]
    assert xyz.shape == (B, A, 3) and elem.shape == (B, A) and n_atoms.shape == (B,)
    ip = lambda a: a.ctypes.data_as(IP)
    dp = lambda a: a.ctypes.data_as(DP)
    return (B, A, dp(xyz), ip(elem), ip(n_atoms), int(flags), float(covalency_factor), int(max_rings), ip(out["status"]),
            ip(out["n_rings"]), ip(out["ring_size"]), ip(out["ring_atoms"]), ip(out["ring_type"]), dp(out["centre"]),
            ip(out["n_orient"]), dp(out["orient"]), out["adj"].ctypes.data_as(C.POINTER(C.c_uint8)))


def host_atoms_to_rings(tables, xyz, elem, n_atoms, flags=0, covalency_factor=1.3, max_rings=RINGS_MAX_RINGS) -> dict:
    """gaudi_host_atoms_to_rings (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = rings_outputs(xyz.shape[0], max_rings)
    rc = lib.gaudi_host_atoms_to_rings(C.byref(tables), *rings_args(xyz, elem, n_atoms, flags, covalency_factor, max_rings, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_atoms_to_rings failed ({rc})")
    return out


def bonds_outputs(B: int, A: int, M: int) -> dict:
    """The four output arrays of gaudi_bond_orders / gaudi_host_bond_orders, in argument order."""
    return dict(order=np.zeros((B, M), np.uint8), charge=np.zeros((B, A), np.int8), n_charged=np.zeros(B, np.int32),
                status=np.zeros(B, np.int32))


def bonds_args(elem, n_atoms, bonds, n_bonds, out):
    """The arguments both entry points share after the tables."""
    for a in (elem, n_atoms, bonds, n_bonds):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    ip = lambda a: a.ctypes.data_as(IP)
    return (B, A, M, ip(elem), ip(n_atoms), ip(bonds), ip(n_bonds), out["order"].ctypes.data_as(C.POINTER(C.c_uint8)),
            out["charge"].ctypes.data_as(C.POINTER(C.c_int8)), ip(out["n_charged"]), ip(out["status"]))


def host_bond_orders(tables, elem, n_atoms, bonds, n_bonds) -> dict:
    """gaudi_host_bond_orders (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = bonds_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    rc = lib.gaudi_host_bond_orders(C.byref(tables), *bonds_args(elem, n_atoms, bonds, n_bonds, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_bond_orders failed ({rc})")
    return out


KEKULE_ARRAYS = ("k", "double_count", "n_hex", "hex_atoms", "sextet_count", "fries", "clar", "n_nodes", "status")


def kekule_outputs(B: int, M: int) -> dict:
    """The nine output arrays of gaudi_kekule / gaudi_host_kekule, in argument order."""
    i32 = lambda: np.zeros(B, np.int32)  # noqa: E731
    return dict(k=np.zeros(B, np.int64), double_count=np.zeros((B, M), np.uint32), n_hex=i32(),
                hex_atoms=np.zeros((B, RINGS_MAX_RINGS, 6), np.int32), sextet_count=np.zeros((B, RINGS_MAX_RINGS), np.uint32),
                fries=i32(), clar=i32(), n_nodes=np.zeros(B, np.int64), status=i32())


def kekule_args(elem, n_atoms, bonds, n_bonds, out):
    """The arguments both entry points share after the tables."""
    for a in (elem, n_atoms, bonds, n_bonds):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    assert out["double_count"].shape == (B, M) and out["hex_atoms"].shape == (B, RINGS_MAX_RINGS, 6)
    ip = lambda a: a.ctypes.data_as(IP)  # noqa: E731
    u32 = lambda a: a.ctypes.data_as(U32P)  # noqa: E731
    i64 = lambda a: a.ctypes.data_as(I64P)  # noqa: E731
    return (B, A, M, ip(elem), ip(n_atoms), ip(bonds), ip(n_bonds), i64(out["k"]), u32(out["double_count"]), ip(out["n_hex"]),
            ip(out["hex_atoms"]), u32(out["sextet_count"]), ip(out["fries"]), ip(out["clar"]), i64(out["n_nodes"]), ip(out["status"]))


def host_kekule(tables, elem, n_atoms, bonds, n_bonds) -> dict:
    """gaudi_host_kekule (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = kekule_outputs(elem.shape[0], bonds.shape[1])
    rc = lib.gaudi_host_kekule(C.byref(tables), *kekule_args(elem, n_atoms, bonds, n_bonds, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_kekule failed ({rc})")
    return out


def canon_outputs(B: int, A: int, M: int) -> dict:
    """The seven output arrays of gaudi_canonical_order / gaudi_host_canonical_order, in argument order."""
    return dict(rank=np.zeros((B, A), np.int32), n_heavy=np.zeros(B, np.int32), label=np.zeros((B, A), np.uint8),
                n_hbonds=np.zeros(B, np.int32), cbonds=np.zeros((B, M, 2), np.uint16), nodes=np.zeros(B, np.int32),
                status=np.zeros(B, np.int32))


def canon_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, out):
    """The arguments both entry points share."""
    for a in (elem, n_atoms, bonds, n_bonds):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    ip = lambda a: a.ctypes.data_as(IP)
    return (int(n_elems), int(h_elem), int(c_elem), B, A, M, ip(elem), ip(n_atoms), ip(bonds), ip(n_bonds), ip(out["rank"]),
            ip(out["n_heavy"]), out["label"].ctypes.data_as(C.POINTER(C.c_uint8)), ip(out["n_hbonds"]),
            out["cbonds"].ctypes.data_as(C.POINTER(C.c_uint16)), ip(out["nodes"]), ip(out["status"]))


def host_canonical_order(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds) -> dict:
    """gaudi_host_canonical_order (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = canon_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    rc = lib.gaudi_host_canonical_order(*canon_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_canonical_order failed ({rc})")
    return out


def fp_outputs(B: int, n_bins: int) -> dict:
    """The three output arrays of gaudi_circular_fingerprint / gaudi_host_circular_fingerprint, in argument order."""
    return dict(fp=np.zeros((B, n_bins), np.uint8), total=np.zeros(B, np.int32), status=np.zeros(B, np.int32))


def fp_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, radius, n_bins, out):
    """The arguments both entry points share."""
    for a in (elem, n_atoms, bonds, n_bonds):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    ip = lambda a: a.ctypes.data_as(IP)
    return (int(n_elems), int(h_elem), int(c_elem), B, A, M, ip(elem), ip(n_atoms), ip(bonds), ip(n_bonds), int(radius),
            int(n_bins), out["fp"].ctypes.data_as(U8P), ip(out["total"]), ip(out["status"]))


def host_circular_fingerprint(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, radius=2, n_bins=1024) -> dict:
    """gaudi_host_circular_fingerprint (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = fp_outputs(elem.shape[0], n_bins if n_bins in FP_BINS else 1)
    rc = lib.gaudi_host_circular_fingerprint(*fp_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, radius, n_bins, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_circular_fingerprint failed ({rc})")
    return out


def fp_rows(a) -> np.ndarray:
    """Fingerprint rows as the entry points read them: uint8 [rows, n_bins], contiguous."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise GaudiError(f"fingerprints must be [rows, n_bins], got shape {a.shape}")
    return a


def nearest_outputs(B: int, k: int) -> dict:
    """The three output arrays of gaudi_fp_nearest / gaudi_host_fp_nearest, in argument order."""
    k = max(int(k), 1)
    return dict(idx=np.zeros((B, k), np.int32), common=np.zeros((B, k), np.int32), union=np.zeros((B, k), np.int32))


def host_fp_nearest(q, lib_rows, k=1) -> dict:
    """gaudi_host_fp_nearest (needs no device): plain loops with the kernels' comparison function.  Test surface only."""
    lib = load_library()
    q, lib_rows = fp_rows(q), fp_rows(lib_rows)
    out = nearest_outputs(q.shape[0], k)
    rc = lib.gaudi_host_fp_nearest(q.shape[1], q.shape[0], q.ctypes.data_as(U8P), lib_rows.shape[0], lib_rows.ctypes.data_as(U8P),
                                   int(k), *(out[n].ctypes.data_as(IP) for n in ("idx", "common", "union")))
    if rc != 0:
        raise GaudiError(f"gaudi_host_fp_nearest failed ({rc})")
    return out


FP_MAX_THRESHOLD_DEN = 65536  # include/gaudi_hip.h: gaudi_fp_neighbours
E_CAPACITY = -5               # include/gaudi_hip.h: GAUDI_E_CAPACITY


def fp_threshold(threshold) -> tuple:
    """A similarity threshold as the exact rational (num, den) the entry points compare with: a float becomes
    Fraction(threshold).limit_denominator(65536), a Fraction or a (num, den) pair is taken as given."""
    from fractions import Fraction
    if isinstance(threshold, (tuple, list)):
        num, den = (int(v) for v in threshold)
    else:
        f = threshold if isinstance(threshold, Fraction) else Fraction(float(threshold)).limit_denominator(FP_MAX_THRESHOLD_DEN)
        num, den = f.numerator, f.denominator
    if not (1 <= den <= FP_MAX_THRESHOLD_DEN and 0 <= num <= den):
        raise GaudiError(f"a threshold is num / den with 0 <= num <= den <= {FP_MAX_THRESHOLD_DEN}, got {num} / {den}")
    return num, den


def _fp_fail(fn, rc, check):
    if check is not None:
        check(rc, fn.__name__)
    raise GaudiError(f"{fn.__name__} failed ({rc})")


def fp_neighbours_call(fn, head, rows, num, den, check=None) -> dict:
    """gaudi_fp_neighbours / gaudi_host_fp_neighbours (head = the handle, or nothing) by the capacity protocol: counts and offsets
    first, then the lists into a buffer of exactly offsets[N] entries -> dict(count int32 [N], offsets int64 [N+1], list int32)."""
    rows = fp_rows(rows)
    N = rows.shape[0]
    count, offsets = np.zeros(N, np.int32), np.zeros(N + 1, np.int64)
    args = (*head, rows.shape[1], N, rows.ctypes.data_as(U8P), int(num), int(den), count.ctypes.data_as(IP))
    rc = fn(*args, 0, offsets.ctypes.data_as(I64P), None)
    if rc != 0:
        _fp_fail(fn, rc, check)
    lst = np.zeros(int(offsets[N]), np.int32)
    if len(lst):
        rc = fn(*args, len(lst), offsets.ctypes.data_as(I64P), lst.ctypes.data_as(IP))
        if rc != 0:
            _fp_fail(fn, rc, check)
    return dict(count=count, offsets=offsets, list=lst)


def fp_cluster_call(fn, head, rows, num, den, check=None) -> dict:
    """gaudi_fp_cluster / gaudi_host_fp_cluster -> dict(cluster, centroid, size, count: int32 [N]; n_clusters int)."""
    rows = fp_rows(rows)
    N = rows.shape[0]
    out = dict(cluster=np.full(N, -1, np.int32), centroid=np.full(N, -1, np.int32), size=np.zeros(N, np.int32),
               count=np.zeros(N, np.int32))
    n = np.zeros(1, np.int32)
    rc = fn(*head, rows.shape[1], N, rows.ctypes.data_as(U8P), int(num), int(den),
            *(out[k].ctypes.data_as(IP) for k in ("cluster", "centroid", "size", "count")), n.ctypes.data_as(IP))
    if rc != 0:
        _fp_fail(fn, rc, check)
    out["n_clusters"] = int(n[0])
    return out


def fp_pick_call(fn, head, rows, S, seeds, first, k, num, den, check=None) -> dict:
    """gaudi_fp_pick_diverse / gaudi_host_fp_pick_diverse.  seeds: rows [S,n_bins] or None (S > 0 then names the resident
    library); first: -1 or a row; den = 0: no threshold -> dict(picked, pick_common, pick_union: int32 [k]; n_picked int; owner,
    owner_common, owner_union: int32 [N])."""
    rows = fp_rows(rows)
    N, k = rows.shape[0], int(k)
    seeds = None if seeds is None else fp_rows(seeds)
    if seeds is not None and (seeds.shape[0] != S or (S and seeds.shape[1] != rows.shape[1])):
        raise GaudiError(f"seeds must be [{S}, {rows.shape[1]}], got {seeds.shape}")
    out = dict(picked=np.full(max(k, 0), -1, np.int32), pick_common=np.zeros(max(k, 0), np.int32), pick_union=np.zeros(max(k, 0), np.int32),
               owner=np.full(N, -1, np.int32), owner_common=np.zeros(N, np.int32), owner_union=np.zeros(N, np.int32))
    n = np.zeros(1, np.int32)
    ip = lambda a: a.ctypes.data_as(IP)  # noqa: E731
    rc = fn(*head, rows.shape[1], N, rows.ctypes.data_as(U8P), int(S), None if seeds is None or S == 0 else seeds.ctypes.data_as(U8P),
            int(first), k, int(num), int(den), ip(out["picked"]), ip(out["pick_common"]), ip(out["pick_union"]), ip(n),
            ip(out["owner"]), ip(out["owner_common"]), ip(out["owner_union"]))
    if rc != 0:
        _fp_fail(fn, rc, check)
    out["n_picked"] = int(n[0])
    return out


def host_fp_neighbours(rows, num, den) -> dict:
    """gaudi_host_fp_neighbours (needs no device): plain loops over every pair.  Test surface only."""
    return fp_neighbours_call(load_library().gaudi_host_fp_neighbours, (), rows, num, den)


def host_fp_cluster(rows, num, den) -> dict:
    """gaudi_host_fp_cluster (needs no device): the literal sort and walk on the host's neighbour lists.  Test surface only."""
    return fp_cluster_call(load_library().gaudi_host_fp_cluster, (), rows, num, den)


def host_fp_pick_diverse(rows, k, num=0, den=0, seeds=None, first=-1) -> dict:
    """gaudi_host_fp_pick_diverse (needs no device): the literal MaxMin loop.  Test surface only."""
    return fp_pick_call(load_library().gaudi_host_fp_pick_diverse, (), rows, 0 if seeds is None else len(seeds), seeds, first, k, num, den)


def sub_outputs(B: int, P: int, A: int, QA: int) -> dict:
    """The five output arrays of gaudi_substructure_search / gaudi_host_substructure_search, in argument order."""
    return dict(count=np.zeros((B, P), np.int32), first=np.full((B, P, QA), -1, np.int32), covered=np.zeros((B, P, A), np.uint8),
                steps=np.zeros((B, P), np.int32), status=np.zeros((B, P), np.int32))


def sub_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, p_elem, p_n_atoms, p_bonds, p_n_bonds, p_flags, out):
    """The arguments both entry points share: the molecules, then the patterns in the same layout, then the outputs."""
    for a in (elem, n_atoms, bonds, n_bonds, p_elem, p_n_atoms, p_bonds, p_n_bonds, p_flags):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    P, QA, QM = p_elem.shape[0], p_elem.shape[1], p_bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    assert p_elem.shape == (P, QA) and p_bonds.shape == (P, QM, 2) and p_n_atoms.shape == (P,) and p_n_bonds.shape == (P,)
    assert p_flags.shape == (P,) and out["count"].shape == (B, P) and out["first"].shape == (B, P, QA) and out["covered"].shape == (B, P, A)
    ip = lambda a: a.ctypes.data_as(IP)
    return (int(n_elems), int(h_elem), int(c_elem), B, A, M, ip(elem), ip(n_atoms), ip(bonds), ip(n_bonds), P, QA, QM, ip(p_elem),
            ip(p_n_atoms), ip(p_bonds), ip(p_n_bonds), ip(p_flags), ip(out["count"]), ip(out["first"]),
            out["covered"].ctypes.data_as(U8P), ip(out["steps"]), ip(out["status"]))


def host_substructure_search(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, p_elem, p_n_atoms, p_bonds, p_n_bonds,
                             p_flags) -> dict:
    """gaudi_host_substructure_search (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = sub_outputs(elem.shape[0], p_elem.shape[0], elem.shape[1], p_elem.shape[1])
    rc = lib.gaudi_host_substructure_search(*sub_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, p_elem, p_n_atoms,
                                                      p_bonds, p_n_bonds, p_flags, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_substructure_search failed ({rc})")
    return out


def host_substructure_root_steps(reset=False) -> int:
    """gaudi_host_substructure_root_steps: the largest per-root step count of the host build since the last reset."""
    return int(load_library().gaudi_host_substructure_root_steps(int(bool(reset))))


HUCKEL_ARRAYS = ("levels", "occupation", "n_pi", "n_electrons", "n_excluded", "sweeps", "flags", "status", "homo", "lumo", "gap",
                 "e_pi", "pi_charge", "pi_bond_order", "site_class")


def huckel_outputs(B: int, A: int, M: int) -> dict:
    """The fifteen output arrays of gaudi_huckel / gaudi_host_huckel, in argument order."""
    i32, f32_ = (lambda: np.zeros(B, np.int32)), (lambda: np.zeros(B, np.float32))
    return dict(levels=np.zeros((B, HUCKEL_MAX_PI), np.float32), occupation=np.zeros((B, HUCKEL_MAX_PI), np.uint8), n_pi=i32(),
                n_electrons=i32(), n_excluded=i32(), sweeps=i32(), flags=i32(), status=i32(), homo=f32_(), lumo=f32_(), gap=f32_(),
                e_pi=f32_(), pi_charge=np.zeros((B, A), np.float32), pi_bond_order=np.zeros((B, M), np.float32),
                site_class=np.zeros((B, A), np.int8))


def huckel_args(tables, elem, n_atoms, bonds, n_bonds, charge, out):
    """The arguments both entry points share: the table, the molecules as bond_orders takes them, charge [B] int32 or None, the
    outputs."""
    for a in (elem, n_atoms, bonds, n_bonds) + (() if charge is None else (charge,)):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    assert charge is None or charge.shape == (B,)
    assert out["levels"].shape == (B, HUCKEL_MAX_PI) and out["pi_charge"].shape == (B, A) and out["pi_bond_order"].shape == (B, M)
    ip = lambda a: a.ctypes.data_as(IP)
    fp = lambda a: a.ctypes.data_as(FP)
    return (C.byref(tables), B, A, M, ip(elem), ip(n_atoms), ip(bonds), ip(n_bonds), None if charge is None else ip(charge),
            fp(out["levels"]), out["occupation"].ctypes.data_as(U8P), ip(out["n_pi"]), ip(out["n_electrons"]), ip(out["n_excluded"]),
            ip(out["sweeps"]), ip(out["flags"]), ip(out["status"]), fp(out["homo"]), fp(out["lumo"]), fp(out["gap"]), fp(out["e_pi"]),
            fp(out["pi_charge"]), fp(out["pi_bond_order"]), out["site_class"].ctypes.data_as(C.POINTER(C.c_int8)))


def host_huckel(tables, elem, n_atoms, bonds, n_bonds, charge=None) -> dict:
    """gaudi_host_huckel (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = huckel_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    rc = lib.gaudi_host_huckel(*huckel_args(tables, elem, n_atoms, bonds, n_bonds, charge, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_huckel failed ({rc})")
    return out


RING_CURRENT_ARRAYS = ("bond_current", "n_rings", "ring_atoms", "ring_size", "ring_current", "ring_area", "normal", "rms_out_of_plane",
                       "gap", "residual", "n_pi", "n_electrons", "sweeps", "flags", "status")
_RING_CURRENT_INT = ("n_rings", "ring_atoms", "ring_size", "n_pi", "n_electrons", "sweeps", "flags", "status")


def ring_current_outputs(B: int, M: int) -> dict:
    """The fifteen output arrays of gaudi_ring_currents / gaudi_host_ring_currents, in argument order."""
    R, S = RING_CURRENT_MAX_RINGS, RING_CURRENT_MAX_SIZE
    shape = dict(bond_current=(B, M), ring_atoms=(B, R, S), ring_size=(B, R), ring_current=(B, R), ring_area=(B, R), normal=(B, 3))
    return {k: np.zeros(shape.get(k, (B,)), np.int32 if k in _RING_CURRENT_INT else np.float32) for k in RING_CURRENT_ARRAYS}


def ring_current_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, out):
    """The arguments both entry points share: the Hueckel table, the molecules as bond_orders takes them, xyz [B,A,3] float32,
    charge [B] int32 or None, the outputs."""
    for a in (elem, n_atoms, bonds, n_bonds) + (() if charge is None else (charge,)):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    assert xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"] and xyz.shape == (B, A, 3)
    assert charge is None or charge.shape == (B,)
    assert out["bond_current"].shape == (B, M) and out["ring_atoms"].shape == (B, RING_CURRENT_MAX_RINGS, RING_CURRENT_MAX_SIZE)
    ptr = lambda k: out[k].ctypes.data_as(IP if k in _RING_CURRENT_INT else FP)
    return ((C.byref(tables), B, A, M, elem.ctypes.data_as(IP), n_atoms.ctypes.data_as(IP), bonds.ctypes.data_as(IP),
             n_bonds.ctypes.data_as(IP), xyz.ctypes.data_as(FP), None if charge is None else charge.ctypes.data_as(IP))
            + tuple(ptr(k) for k in RING_CURRENT_ARRAYS))


def host_ring_currents(tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None) -> dict:
    """gaudi_host_ring_currents (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = ring_current_outputs(elem.shape[0], bonds.shape[1])
    rc = lib.gaudi_host_ring_currents(*ring_current_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_ring_currents failed ({rc})")
    return out


REACTIVITY_ARRAYS = ("atom_localization", "free_valence", "rings", "n_rings", "para_localization", "ortho_localization", "e_pi",
                     "n_pi", "n_electrons", "n_jobs", "sweeps", "flags", "status")
_REACTIVITY_INT = ("rings", "n_rings", "n_pi", "n_electrons", "n_jobs", "sweeps", "flags", "status")


def reactivity_outputs(B: int, A: int, M: int) -> dict:
    """The thirteen output arrays of gaudi_reactivity / gaudi_host_reactivity, in argument order."""
    R, S = RING_CURRENT_MAX_RINGS, RING_CURRENT_MAX_SIZE
    shape = dict(atom_localization=(B, REACTIVITY_KINDS, A), free_valence=(B, A), rings=(B, R, S), para_localization=(B, R, 3),
                 ortho_localization=(B, M))
    return {k: np.zeros(shape.get(k, (B,)), np.int32 if k in _REACTIVITY_INT else np.float32) for k in REACTIVITY_ARRAYS}


def reactivity_args(tables, elem, n_atoms, bonds, n_bonds, charge, with_bonds, slices, out):
    """The arguments both entry points share: the Hueckel table, the molecules as bond_orders takes them, charge [B] int32 or None,
    with_bonds, slices (0: the entry point chooses), the outputs."""
    for a in (elem, n_atoms, bonds, n_bonds) + (() if charge is None else (charge,)):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    assert charge is None or charge.shape == (B,)
    assert out["atom_localization"].shape == (B, REACTIVITY_KINDS, A) and out["ortho_localization"].shape == (B, M)
    ptr = lambda k: out[k].ctypes.data_as(IP if k in _REACTIVITY_INT else FP)
    return ((C.byref(tables), B, A, M, elem.ctypes.data_as(IP), n_atoms.ctypes.data_as(IP), bonds.ctypes.data_as(IP),
             n_bonds.ctypes.data_as(IP), None if charge is None else charge.ctypes.data_as(IP), int(bool(with_bonds)), int(slices))
            + tuple(ptr(k) for k in REACTIVITY_ARRAYS))


def host_reactivity(tables, elem, n_atoms, bonds, n_bonds, charge=None, with_bonds=True, slices=0) -> dict:
    """gaudi_host_reactivity (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = reactivity_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    rc = lib.gaudi_host_reactivity(*reactivity_args(tables, elem, n_atoms, bonds, n_bonds, charge, with_bonds, slices, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_reactivity failed ({rc})")
    return out


PPP_ARRAYS = ("levels", "occupation", "pi_charge", "pi_bond_order", "site_class", "n_pi", "n_electrons", "n_excluded", "iterations",
              "sweeps", "flags", "status", "homo", "lumo", "gap", "e_electronic", "e_core", "delta_p")


def ppp_outputs(B: int, A: int, M: int) -> dict:
    """The eighteen output arrays of gaudi_ppp / gaudi_host_ppp, in argument order."""
    out = dict(levels=np.zeros((B, HUCKEL_MAX_PI), np.float32), occupation=np.zeros((B, HUCKEL_MAX_PI), np.uint8),
               pi_charge=np.zeros((B, A), np.float32), pi_bond_order=np.zeros((B, M), np.float32), site_class=np.zeros((B, A), np.int8))
    out.update({k: np.zeros(B, np.int32) for k in PPP_ARRAYS[5:12]})
    out.update({k: np.zeros(B, np.float32) for k in PPP_ARRAYS[12:]})
    return out


def ppp_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, repulsion, damping, out):
    """The arguments both entry points share: the table, the molecules as bond_orders takes them, xyz [B,A,3] float32, charge [B]
    int32 or None, the repulsion formula (PPP_MATAGA_NISHIMOTO / PPP_OHNO), the damping, the outputs."""
    for a in (elem, n_atoms, bonds, n_bonds) + (() if charge is None else (charge,)):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    B, A, M = elem.shape[0], elem.shape[1], bonds.shape[1]
    assert elem.shape == (B, A) and bonds.shape == (B, M, 2) and n_atoms.shape == (B,) and n_bonds.shape == (B,)
    assert xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"] and xyz.shape == (B, A, 3)
    assert charge is None or charge.shape == (B,)
    assert out["levels"].shape == (B, HUCKEL_MAX_PI) and out["pi_charge"].shape == (B, A) and out["pi_bond_order"].shape == (B, M)
    ip = lambda a: a.ctypes.data_as(IP)
    fp = lambda a: a.ctypes.data_as(FP)
    return ((C.byref(tables), B, A, M, ip(elem), ip(n_atoms), ip(bonds), ip(n_bonds), fp(xyz), None if charge is None else ip(charge),
             int(repulsion), float(damping), fp(out["levels"]), out["occupation"].ctypes.data_as(U8P), fp(out["pi_charge"]),
             fp(out["pi_bond_order"]), out["site_class"].ctypes.data_as(C.POINTER(C.c_int8)))
            + tuple(ip(out[k]) for k in PPP_ARRAYS[5:12]) + tuple(fp(out[k]) for k in PPP_ARRAYS[12:]))


def host_ppp(tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, repulsion=PPP_MATAGA_NISHIMOTO, damping=0.25) -> dict:
    """gaudi_host_ppp (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = ppp_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    rc = lib.gaudi_host_ppp(*ppp_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, repulsion, damping, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_ppp failed ({rc})")
    return out


PPP_OPEN_ARRAYS = PPP_ARRAYS + ("spin_density", "e_state", "he_correction", "n_open", "somo")


def ppp_open_outputs(B: int, A: int, M: int) -> dict:
    """The twenty-three output arrays of gaudi_ppp_open / gaudi_host_ppp_open, in argument order."""
    out = ppp_outputs(B, A, M)
    out.update(spin_density=np.zeros((B, A), np.float32), e_state=np.zeros(B, np.float64), he_correction=np.zeros(B, np.float64),
               n_open=np.zeros(B, np.int32), somo=np.zeros((B, 2), np.int32))
    return out


def ppp_open_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity, repulsion, damping, out):
    """ppp_args with multiplicity [B] int32 or None behind the charge and the five further outputs at the end."""
    base = ppp_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, repulsion, damping, out)
    B, A = elem.shape
    assert multiplicity is None or (multiplicity.dtype == np.int32 and multiplicity.flags["C_CONTIGUOUS"] and multiplicity.shape == (B,))
    assert out["spin_density"].shape == (B, A) and out["somo"].shape == (B, 2)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    return (base[:10] + (None if multiplicity is None else multiplicity.ctypes.data_as(IP),) + base[10:]
            + (out["spin_density"].ctypes.data_as(FP), dp(out["e_state"]), dp(out["he_correction"]), out["n_open"].ctypes.data_as(IP),
               out["somo"].ctypes.data_as(IP)))


def host_ppp_open(tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, multiplicity=None, repulsion=PPP_MATAGA_NISHIMOTO,
                  damping=0.25) -> dict:
    """gaudi_host_ppp_open (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = ppp_open_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    rc = lib.gaudi_host_ppp_open(*ppp_open_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity, repulsion, damping, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_ppp_open failed ({rc})")
    return out


PPP_SCF_ARRAYS = PPP_OPEN_ARRAYS + ("diis_error", "n_extrapolated")
PPP_DIIS_MAX, PPP_DIIS_ERROR = 8, 2.0 ** -10


def ppp_scf_outputs(B: int, A: int, M: int) -> dict:
    """The twenty-five output arrays of gaudi_ppp_scf / gaudi_host_ppp_scf, in argument order."""
    out = ppp_open_outputs(B, A, M)
    out.update(diis_error=np.zeros(B, np.float32), n_extrapolated=np.zeros(B, np.int32))
    return out


def ppp_scf_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity, repulsion, diis_size, diis_start, damping, out):
    """ppp_open_args with the history's length and its first iteration in front of the damping and the two further outputs at the end."""
    base = ppp_open_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity, repulsion, damping, out)
    assert out["diis_error"].shape == out["n_extrapolated"].shape == (elem.shape[0],)
    return base[:12] + (int(diis_size), int(diis_start)) + base[12:] + (out["diis_error"].ctypes.data_as(FP), out["n_extrapolated"].ctypes.data_as(IP))


def host_ppp_scf(tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, multiplicity=None, repulsion=PPP_MATAGA_NISHIMOTO, diis_size=6,
                 diis_start=3, damping=0.25) -> dict:
    """gaudi_host_ppp_scf (needs no device): the kernel's source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = ppp_scf_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    rc = lib.gaudi_host_ppp_scf(*ppp_scf_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity, repulsion, diis_size,
                                              diis_start, damping, out))
    if rc != 0:
        raise GaudiError(f"gaudi_host_ppp_scf failed ({rc})")
    return out


PPP_CIS_ARRAYS = ("singlet", "triplet", "osc", "dipole", "lead", "lead_weight", "n_states", "n_active_occ", "n_active_virt",
                  "cis_sweeps")


def ppp_cis_outputs(B: int) -> dict:
    """The ten output arrays gaudi_ppp_cis / gaudi_host_ppp_cis add to gaudi_ppp's eighteen, in argument order."""
    S = PPP_CIS_MAX_STATES
    out = dict(singlet=np.zeros((B, S), np.float32), triplet=np.zeros((B, S), np.float32), osc=np.zeros((B, S), np.float32),
               dipole=np.zeros((B, S, 3), np.float32), lead=np.zeros((B, S, 2), np.uint8), lead_weight=np.zeros((B, S), np.float32))
    out.update({k: np.zeros(B, np.int32) for k in PPP_CIS_ARRAYS[6:]})
    return out


def ppp_cis_args(window, out):
    """What follows ppp_args: the window and the ten CIS outputs."""
    fp = lambda a: a.ctypes.data_as(FP)
    return ((int(window),) + tuple(fp(out[k]) for k in PPP_CIS_ARRAYS[:4]) + (out["lead"].ctypes.data_as(U8P), fp(out["lead_weight"]))
            + tuple(out[k].ctypes.data_as(IP) for k in PPP_CIS_ARRAYS[6:]))


def host_ppp_cis(tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, repulsion=PPP_MATAGA_NISHIMOTO, damping=0.25,
                 window=PPP_CIS_MAX_WINDOW) -> dict:
    """gaudi_host_ppp_cis (needs no device): the two kernels' source text run serially on the host.  Test surface only."""
    lib = load_library()
    out = ppp_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
    out.update(ppp_cis_outputs(elem.shape[0]))
    rc = lib.gaudi_host_ppp_cis(*(ppp_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, repulsion, damping, out)
                                  + ppp_cis_args(window, out)))
    if rc != 0:
        raise GaudiError(f"gaudi_host_ppp_cis failed ({rc})")
    return out


def fptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(FP)


def f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def grid_coefficients(T: int, noise_power: float, noise_precision: float, grid):
    """The step table of a time grid as the chains build it (include/gaudi_hip.h: gaudi_host_grid_coefficients; needs no
    device) -> (coef [n-1,4] = alpha_t|s, sigma2_t|s / alpha_t|s / sigma_t, sigma, t of step g[k] -> g[k+1];
    land [n-1] = the time index each step lands on)."""
    lib = load_library()
    g = np.ascontiguousarray(np.asarray(grid).reshape(-1), dtype=np.int32)
    coef = np.zeros((max(len(g) - 1, 0), 4), np.float32)
    land = np.zeros(max(len(g) - 1, 0), np.int32)
    rc = lib.gaudi_host_grid_coefficients(int(T), float(noise_power), float(noise_precision), len(g), g.ctypes.data_as(IP),
                                          coef.ctypes.data_as(FP), land.ctypes.data_as(IP))
    if rc != 0:
        raise GaudiError(f"gaudi_host_grid_coefficients failed ({rc}): the grid must be strictly descending integers "
                         f"T >= g[0] > ... > g[n] = 0 with at least two entries")
    return coef, land
