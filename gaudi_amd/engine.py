"""Thin object wrapper over the C ABI: one Engine = one gaudi_handle = one GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import TARGET_CB, TARGET_CBZ, Diag, EdmConfig, GaudiError, PredConfig, f32, fptr


def _strip(sd: dict) -> dict:
    """Checkpoints saved with dp=True carry a ``module.`` prefix (models_edm.py:98-102)."""
    out = {}
    for k, v in sd.items():
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        out[k[7:] if k.startswith("module.") else k] = f32(v)
    return out


def _noise_power(schedule: str) -> float:
    """-> gaudi_edm_config.noise_power: p of 'polynomial_<p>', 0 for 'cosine' (PredefinedNoiseSchedule, en_diffusion.py:191-202)."""
    if schedule == "cosine":
        return 0.0
    parts = str(schedule).split("_")
    try:
        power = float(parts[1]) if len(parts) == 2 and parts[0] == "polynomial" else 0.0
    except ValueError:  # 'polynomial_x'
        power = 0.0
    if not power > 0:
        raise GaudiError(f"unsupported diffusion_noise_schedule {schedule!r}: 'polynomial_<p>' and 'cosine' are implemented "
                         "(the 'learned' schedule is training-only in the reference)")
    return power


def target_spec(spec, B: int, K: int):
    """A value-target spec (dict with any of w, q, c, side, scale, window; include/gaudi_hip.h: gaudi_target_spec) as the C
    struct -> (struct, arrays it points into: keep them alive for the call).  w / q / c / side: [K] shared or [B,K] per
    molecule; scale: a float or [B]; window = (t_lo, t_hi) time indices, None = every step.  Shapes are checked here, values
    (sides, finiteness, the window against T) by the library."""
    if not isinstance(spec, dict):
        if callable(getattr(spec, "spec", None)):  # a models_edm.ValueTarget
            spec = spec.spec()
        else:
            raise GaudiError("a target spec is a dict with any of w, q, c, side, scale, window (or a ValueTarget), "
                             f"got {type(spec).__name__}")
    unknown = set(spec) - {"w", "q", "c", "side", "scale", "window"}
    if unknown:
        raise GaudiError(f"unknown target spec entries {sorted(unknown)}")
    cs = _lib.TargetSpec()
    keep = []

    def arr(name, dtype):
        a = spec.get(name)
        if a is None:
            return None, 0
        a = np.ascontiguousarray(np.asarray(a), dtype=dtype)
        if a.shape == (K,):
            per = 0
        elif a.shape == (B, K):
            per = 1
        else:
            raise GaudiError(f"target spec '{name}' must be [K] = {(K,)} or [B,K] = {(B, K)}, got {a.shape}")
        keep.append(a)
        return a, per

    cs.K = K
    for name in ("w", "q", "c"):
        a, per = arr(name, np.float32)
        setattr(cs, name, None if a is None else a.ctypes.data_as(_lib.FP))
        setattr(cs, name + "_per_mol", per)
    sd = spec.get("side")
    if sd is not None and not np.all(np.asarray(sd) == np.round(np.asarray(sd, np.float64))):
        raise GaudiError("target spec 'side' must hold -1 (lower bound), 0 (value) or +1 (upper bound)")
    a, per = arr("side", np.int32)
    cs.side = None if a is None else a.ctypes.data_as(_lib.IP)
    cs.side_per_mol = per
    sc = spec.get("scale")
    if sc is not None:
        per = np.ndim(sc) > 0  # a number is shared; an array holds one scale per molecule and must have B entries
        sc = np.asarray(sc, np.float32)
        if sc.shape != ((B,) if per else ()):
            raise GaudiError(f"target spec 'scale' must be a number or [B] = {(B,)}, got {sc.shape}")
        sc = np.ascontiguousarray(sc.reshape(-1))
        keep.append(sc)
        cs.scale = sc.ctypes.data_as(_lib.FP)
        cs.scale_per_mol = 1 if per else 0
    win = spec.get("window")
    if win is not None:
        cs.t_lo, cs.t_hi = int(win[0]), int(win[1])
        if cs.t_lo == 0 and cs.t_hi == 0:
            raise GaudiError("the guidance window must lie inside 1..T")
    return cs, keep


def host_target_seed(spec, pred) -> np.ndarray:
    """d(scale_b T_b)/dpred [B,K] of a value-target spec at pred [B,K], by the function the kernels use (no device;
    include/gaudi_hip.h: gaudi_host_target_seed)."""
    p = f32(pred)
    if p.ndim != 2:
        raise GaudiError(f"pred must be [B,K], got {p.shape}")
    B, K = p.shape
    cs, keep = target_spec(spec, B, K)
    out = np.empty_like(p)
    rc = _lib.load_library().gaudi_host_target_seed(C.byref(cs), B, K, fptr(p), fptr(out))
    del keep
    if rc != 0:
        raise GaudiError(f"gaudi_host_target_seed failed ({rc}): side must be -1 / 0 / +1 and every parameter finite")
    return out


class Engine:
    def __init__(self, device: int = 0):
        self.lib = _lib.load_library()
        self.h = C.c_void_p()
        rc = self.lib.gaudi_create(int(device), C.byref(self.h))
        if rc != 0:
            raise GaudiError(f"gaudi_create(device={device}) failed with code {rc} (no usable HIP device?)")
        self.device = device
        self.edm_args = None
        self.pred_args = None
        self.fix_noise = False
        self.F = None
        self.K = None

    _default = None

    @classmethod
    def default(cls, device: int = 0) -> "Engine":
        """Process-wide handle for calls that need no weights (stability check); created on first use."""
        if cls._default is None or not cls._default.h:
            cls._default = cls(device)
        return cls._default

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.gaudi_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _warning(self):
        """The library's last non-fatal condition ('' if none, or an older A/B library without the entry point)."""
        fn = getattr(self.lib, "gaudi_last_warning", None)
        if fn is None or fn.restype is not C.c_char_p:
            return ""
        msg = fn(self.h)
        return msg.decode() if msg else ""

    def _note_fallback(self):
        """A weight set the fp16-pair images refuse runs the fp32-instruction kernels at about 0.55 x the speed: say so once,
        loudly, and keep the reason for diag['edge_math_fallback']."""
        w = self._warning()
        if w and w != getattr(self, "_fallback_reason", None):
            import warnings
            warnings.warn("gaudi_amd: " + w, RuntimeWarning, stacklevel=3)
        if w:
            self._fallback_reason = w

    def profile_clock_mhz(self) -> float:
        """Shader clock the chip held during the most recent profiled sampler launch (0.0: none, or an older A/B library)."""
        fn = getattr(self.lib, "gaudi_profile_clock", None)
        if fn is None or not fn.argtypes:
            return 0.0
        v = C.c_double(0.0)
        self._check(fn(self.h, C.byref(v)), "gaudi_profile_clock")
        return float(v.value)

    def last_kernel_key(self) -> str:
        """The kernel-table key of the kernel the most recent launch ran, e.g. 'waves=8 SP=1 ... N1=1 ... VT=0' ('' before the
        first launch, or an older A/B library without the entry point)."""
        fn = getattr(self.lib, "gaudi_last_kernel_key", None)
        if fn is None or not fn.argtypes:
            return ""
        buf = C.create_string_buffer(256)
        self._check(fn(self.h, buf, len(buf)), "gaudi_last_kernel_key")
        return buf.value.decode()

    def kernel_keys_launched(self) -> list:
        """The distinct kernel-table keys this engine has launched since it was made, in first-launch order (a call may be two
        launches: the 4-wave global-node-buffer kernels, a sin_embedding width without a fused kernel)."""
        fn = getattr(self.lib, "gaudi_kernel_key_log", None)
        if fn is None or not fn.argtypes:  # (an older A/B library)
            return []
        return _lib.key_lines(fn, self.h)

    def keep_h(self) -> int:
        """Floats of LDS the most recent call gave to a kept split copy of h (0: none)."""
        fn = getattr(self.lib, "gaudi_last_keep_h", None)
        if fn is None or not fn.argtypes:
            return 0
        n = C.c_int32(0)
        self._check(fn(self.h, C.byref(n)), "gaudi_last_keep_h")
        return int(n.value)

    def family_split(self) -> int:
        """Molecules of the most recent sample() call that ran on the resident kernels beside a V8G bucket (0: one family)."""
        fn = getattr(self.lib, "gaudi_last_family_split", None)
        if fn is None or not fn.argtypes:
            return 0
        n = C.c_int32(0)
        self._check(fn(self.h, C.byref(n)), "gaudi_last_family_split")
        return int(n.value)

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.gaudi_last_error(self.h)
            raise GaudiError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _tensor_args(self, sd: dict):
        names = list(sd.keys())
        arrs = [sd[k] for k in names]
        n = len(names)
        c_names = (C.c_char_p * n)(*[k.encode() for k in names])
        c_ptrs = (_lib.FP * n)(*[fptr(a) for a in arrs])
        c_numel = (C.c_int64 * n)(*[a.size for a in arrs])
        return n, c_names, c_ptrs, c_numel, arrs

    # ------------------------------------------------------------------ weights
    def load_edm(self, args: dict, state_dict: dict):
        """args: the checkpoint's args.txt namespace (utils/args_edm.py); state_dict: model.pt."""
        agg = args.get("aggregation_method", "sum")
        if agg not in ("sum", "mean"):
            raise GaudiError(f"unknown aggregation_method {agg!r}")
        sd = _strip(state_dict)
        emb = sd.get("dynamics.egnn.embedding.weight")
        if emb is None:
            raise GaudiError("state dict has no dynamics.egnn.embedding.weight (mode='gnn_dynamics' is unsupported)")
        F = emb.shape[1] - 1  # in_node_nf is not stored: recover it
        from .checkpoint import normalize_factors
        nv = normalize_factors(args)
        cfg = EdmConfig(F, int(args["nf"]), int(args["n_layers"]), int(args.get("inv_sublayers", 1)),
                        int(bool(args["attention"])), int(bool(args["tanh"])), float(args["coords_range"]),
                        float(args["norm_constant"]), float(args.get("normalization_factor", 1)) if agg == "sum" else 0.0,
                        int(args["diffusion_steps"]), _noise_power(args["diffusion_noise_schedule"]),
                        float(args["diffusion_noise_precision"]), (C.c_float * 3)(*[float(v) for v in nv]),
                        int(bool(args.get("sin_embedding", False))))
        n, c_names, c_ptrs, c_numel, keep = self._tensor_args(sd)
        self._check(self.lib.gaudi_load_edm(self.h, C.byref(cfg), n, c_names, c_ptrs, c_numel), "gaudi_load_edm")
        self._note_fallback()
        self.edm_args, self.F, self.T = dict(args), F, int(args["diffusion_steps"])
        self.edm_names = list(sd.keys())
        self.edm_shapes = [sd[k].shape for k in self.edm_names]
        self._edm_train_sd = None  # weights given to edm_set_train_weights since this load (the sampler images lag behind)
        # EnVariationalDiffusion.check_issues_norm_values (en_diffusion.py:336-349): the reference refuses to BUILD a model whose
        # sigma_0 is not small against 1 / norm_value (8 standard deviations) -- e.g. 'cosine' with the default
        # normalize_factors [3, 4, 10]; a checkpoint it could never have produced is refused here as well
        sigma_0 = float(np.sqrt(1.0 / (1.0 + np.exp(-np.float64(self.gamma()[0])))))
        max_norm = max(float(nv[1]), float(nv[2]))
        if sigma_0 * 8 > 1.0 / max_norm:
            raise GaudiError(f"Value for normalization value {max_norm} probably too large with sigma_0 {sigma_0:.5f} and "
                             f"1 / norm_value = {1.0 / max_norm} (en_diffusion.py:336-349: the reference raises the same)")

    def load_predictor(self, args: dict, state_dict: dict):
        sd = _strip(state_dict)
        emb = sd["egnn.embedding.weight"]
        F = emb.shape[1] - 1
        K = sd["egnn.embedding_out.weight"].shape[0]
        cfg = PredConfig(F, K, int(args["nf"]), int(args["n_layers"]), int(bool(args["attention"])),
                         int(bool(args["tanh"])), float(args["coords_range"]))
        n, c_names, c_ptrs, c_numel, keep = self._tensor_args(sd)
        self._check(self.lib.gaudi_load_predictor(self.h, C.byref(cfg), n, c_names, c_ptrs, c_numel),
                    "gaudi_load_predictor")
        # a reload reports the weights now loaded: a predictor fallback of the previous weights no longer holds
        reason = getattr(self, "_fallback_reason", None)
        if reason and reason.startswith("predictor weights") and self._warning() != reason:
            self._fallback_reason = None
        self._note_fallback()
        self.pred_args, self.K = dict(args), K
        self.pred_names = list(sd.keys())
        self.pred_shapes = [sd[k].shape for k in self.pred_names]

    edm_sync = None  # set by a GaudiModel: pushes parameters an optimizer changed (edm_set_train_weights) before an EDM call

    def _sync_edm(self, sampler: bool = True):
        """Before an EDM call: let the model push changed parameters; before a sampler-kernel call (sampler=True) also
        rebuild the sampler's images with load_edm when edm_set_train_weights has left them stale, once per change."""
        if self.edm_sync is not None:
            self.edm_sync()
        if sampler and getattr(self, "_edm_train_sd", None) is not None:
            sd, self._edm_train_sd = self._edm_train_sd, None
            self.load_edm(self.edm_args, sd)

    pred_sync = None  # set by a trainable CondPredictor: pushes parameters an optimizer changed before any predictor call

    def _sync_pred(self):
        if self.pred_sync is not None:
            self.pred_sync()

    # ------------------------------------------------------------------ tables
    def gamma(self) -> np.ndarray:
        g = np.empty(self.T + 1, np.float32)
        self._check(self.lib.gaudi_get_gamma(self.h, fptr(g)), "gaudi_get_gamma")
        return g

    def step_coefficients(self) -> np.ndarray:
        c = np.empty((self.T, 4), np.float32)
        self._check(self.lib.gaudi_get_step_coefficients(self.h, fptr(c)), "gaudi_get_step_coefficients")
        return c

    # ------------------------------------------------------------------ unit entry points
    @staticmethod
    def _masks(node_mask, edge_mask, B, N):
        nm = f32(node_mask).reshape(B, N)
        em = f32(edge_mask).reshape(B, N, N)
        return nm, em

    def phi(self, z, t, node_mask, edge_mask) -> np.ndarray:
        self._sync_edm()
        z = f32(z)
        B, N, D = z.shape
        nm, em = self._masks(node_mask, edge_mask, B, N)
        t = f32(np.broadcast_to(np.asarray(t, np.float32).reshape(-1), (B,)))
        out = np.empty_like(z)
        self._check(self.lib.gaudi_phi(self.h, B, N, fptr(z), fptr(t), fptr(nm), fptr(em), fptr(out)), "gaudi_phi")
        return out

    def predictor_fwd(self, z, t, node_mask, edge_mask) -> np.ndarray:
        self._sync_pred()
        z = f32(z)
        B, N, D = z.shape
        nm, em = self._masks(node_mask, edge_mask, B, N)
        t = f32(np.broadcast_to(np.asarray(t, np.float32).reshape(-1), (B,)))
        out = np.empty((B, self.K), np.float32)
        self._check(self.lib.gaudi_predictor_fwd(self.h, B, N, fptr(z), fptr(t), fptr(nm), fptr(em), fptr(out)),
                    "gaudi_predictor_fwd")
        return out

    def predictor_grad(self, z, t, node_mask, edge_mask, dpred):
        self._sync_pred()
        z = f32(z)
        B, N, D = z.shape
        nm, em = self._masks(node_mask, edge_mask, B, N)
        t = f32(np.broadcast_to(np.asarray(t, np.float32).reshape(-1), (B,)))
        dp = f32(np.broadcast_to(np.asarray(dpred, np.float32), (B, self.K)))
        pred = np.empty((B, self.K), np.float32)
        grad = np.empty_like(z)
        self._check(self.lib.gaudi_predictor_grad(self.h, B, N, fptr(z), fptr(t), fptr(nm), fptr(em), fptr(dp),
                                                  fptr(pred), fptr(grad)), "gaudi_predictor_grad")
        return pred, grad

    def step(self, s_idx, z_t, node_mask, edge_mask, eps_raw, target_w=None, scale=1.0, t_idx=None) -> np.ndarray:
        """One teacher-forced reverse step z_t -> z_s from time index t_idx (default s_idx + 1) down to s_idx."""
        self._sync_edm()
        self._sync_pred()
        z = f32(z_t)
        B, N, D = z.shape
        nm, em = self._masks(node_mask, edge_mask, B, N)
        eps = f32(eps_raw)
        tw = None if target_w is None else f32(target_w)
        out = np.empty_like(z)
        if t_idx is not None:
            self._check(self.lib.gaudi_step_pair(self.h, B, N, int(s_idx), int(t_idx), fptr(z), fptr(nm), fptr(em), fptr(eps),
                                                 fptr(tw), float(scale), fptr(out)), "gaudi_step_pair")
            return out
        self._check(self.lib.gaudi_step(self.h, B, N, int(s_idx), fptr(z), fptr(nm), fptr(em), fptr(eps), fptr(tw),
                                        float(scale), fptr(out)), "gaudi_step")
        return out

    def decode(self, z0, node_mask, edge_mask, eps_raw):
        self._sync_edm()
        z = f32(z0)
        B, N, D = z.shape
        nm, em = self._masks(node_mask, edge_mask, B, N)
        eps = f32(eps_raw)
        x = np.empty((B, N, 3), np.float32)
        h = np.empty((B, N, D - 3), np.float32)
        self._check(self.lib.gaudi_decode(self.h, B, N, fptr(z), fptr(nm), fptr(em), fptr(eps), fptr(x), fptr(h)),
                    "gaudi_decode")
        return x, h

    # ------------------------------------------------------------------ whole chain
    def _grid_args(self, grid, start, B, N, return_zt):
        """-> (n_grid, grid int32, x0, onehot0, zt) for the *_grid entry points; malformed grids are refused by the library."""
        g = np.ascontiguousarray(np.asarray(grid).reshape(-1), dtype=np.int32)
        x0 = oh0 = zt = None
        if start is not None:
            x0, oh0 = start
            x0 = None if x0 is None else f32(x0).reshape(B, N, 3)
            oh0 = None if oh0 is None else f32(oh0).reshape(B, N, self.F)
            if return_zt:
                zt = np.zeros((B, N, 3 + self.F), np.float32)
        elif return_zt:
            raise GaudiError("return_zt needs a start from given molecules (start=(x, onehot))")
        return len(g), g, x0, oh0, zt

    def sample(self, node_mask, edge_mask, *, seed=0, sample_offset=0, noise=None, std=1.0, target_w=None, scale=1.0,
               return_z0=False, grid=None, start=None, return_zt=False):
        """Whole chain -> (x, h, diag[, z0][, zt]).  grid: strictly descending time indices T >= g[0] > ... > g[n] = 0 (None:
        all T steps); start = (x, onehot): noise these molecules to g[0] and run the chain from there instead of from the
        prior (needs a grid; return_zt also returns that z_{g[0]}).  See include/gaudi_hip.h: gaudi_sample_grid."""
        if grid is None and start is not None:
            raise GaudiError("a start from given molecules needs the time grid to run (grid[0] = the time index to noise to)")
        self._sync_edm()
        self._sync_pred()
        nm = f32(node_mask)
        B, N = nm.shape[0], nm.shape[1]
        nm, em = self._masks(nm, edge_mask, B, N)
        D = 3 + self.F
        nz = None
        if noise is not None:
            nz = f32(noise)
            want = (self.T + 2, 1 if self.fix_noise else B, N, D)
            if nz.shape != want:
                raise GaudiError(f"noise must be [T+2,{'1' if self.fix_noise else 'B'},N,3+F] = {want}, got {nz.shape}")
        tw = None if target_w is None else f32(target_w)
        x = np.empty((B, N, 3), np.float32)
        h = np.empty((B, N, self.F), np.float32)
        z0 = np.empty((B, N, D), np.float32) if return_z0 else None
        diag = Diag()
        zt = None
        if grid is None:
            self._check(self.lib.gaudi_sample(self.h, B, N, fptr(nm), fptr(em), int(seed), int(sample_offset), fptr(nz),
                                              float(std), fptr(tw), float(scale), fptr(x), fptr(h), fptr(z0),
                                              C.byref(diag)), "gaudi_sample")
        else:
            ng, g, x0, oh0, zt = self._grid_args(grid, start, B, N, return_zt)
            self._check(self.lib.gaudi_sample_grid(self.h, B, N, fptr(nm), fptr(em), int(seed), int(sample_offset), fptr(nz),
                                                   float(std), fptr(tw), float(scale), ng, g.ctypes.data_as(_lib.IP), fptr(x0),
                                                   fptr(oh0), fptr(x), fptr(h), fptr(z0), fptr(zt), C.byref(diag)),
                        "gaudi_sample_grid")
        d = dict(max_masked_leak=diag.max_masked_leak, max_cog_rel=diag.max_cog_rel, max_cog_abs=diag.max_cog_abs,
                 nan_count=diag.nan_count, reprojected=diag.reprojected,
                 edge_math_fallback=getattr(self, "_fallback_reason", None), family_split_resident=self.family_split())
        out = (x, h, d) + ((z0,) if return_z0 else ())
        return out + (zt,) if return_zt else out

    def predict_noised(self, x, onehot, t_int, node_mask, edge_mask, *, seed=0, sample_offset=0, noise=None):
        """sample_edm_t + predictor forward in one launch -> (z_t [B,N,3+F], pred [B,K])."""
        self._sync_pred()
        x = f32(x)
        B, N = x.shape[0], x.shape[1]
        oh = f32(onehot).reshape(B, N, self.F)
        nm, em = self._masks(f32(node_mask).reshape(B, N), edge_mask, B, N)
        ti = np.ascontiguousarray(np.broadcast_to(np.asarray(t_int).reshape(-1), (B,)), dtype=np.int32)
        nz = None
        if noise is not None:
            nz = f32(noise)
            if nz.shape != (B, N, 3 + self.F):
                raise GaudiError(f"noise must be [B,N,3+F] = {(B, N, 3 + self.F)}, got {nz.shape}")
        zt = np.empty((B, N, 3 + self.F), np.float32)
        pred = np.empty((B, self.K), np.float32)
        self._check(self.lib.gaudi_predict_noised(self.h, B, N, fptr(x), fptr(oh), ti.ctypes.data_as(_lib.IP), fptr(nm),
                                                  fptr(em), int(seed), int(sample_offset), fptr(nz), fptr(zt),
                                                  fptr(pred)), "gaudi_predict_noised")
        return zt, pred

    def predictor_loss_grad(self, x, onehot, t_int, node_mask, edge_mask, y, *, seed=0, sample_offset=0, noise=None):
        """compute_loss + loss.backward() of the predictor (include/gaudi_hip.h: gaudi_predictor_loss_grad) ->
        (loss, pred [B,K], {name: d loss / d tensor, or None where the tensor has no gradient path}) in the names and
        shapes of the state dict given to load_predictor.  Inputs as predict_noised, plus the targets y [B,K]."""
        self._sync_pred()
        x = f32(x)
        B, N = x.shape[0], x.shape[1]
        oh = f32(onehot).reshape(B, N, self.F)
        nm, em = self._masks(f32(node_mask).reshape(B, N), edge_mask, B, N)
        ti = np.ascontiguousarray(np.broadcast_to(np.asarray(t_int).reshape(-1), (B,)), dtype=np.int32)
        yy = f32(y).reshape(B, self.K)
        nz = None
        if noise is not None:
            nz = f32(noise)
            if nz.shape != (B, N, 3 + self.F):
                raise GaudiError(f"noise must be [B,N,3+F] = {(B, N, 3 + self.F)}, got {nz.shape}")
        n = C.c_int64(0)
        self._check(self.lib.gaudi_predictor_grad_size(self.h, C.byref(n)), "gaudi_predictor_grad_size")
        grad = np.zeros(int(n.value), np.float32)
        has = np.zeros(len(self.pred_names), np.int32)
        loss = np.zeros(1, np.float32)
        pred = np.empty((B, self.K), np.float32)
        self._check(self.lib.gaudi_predictor_loss_grad(self.h, B, N, fptr(x), fptr(oh), ti.ctypes.data_as(_lib.IP), fptr(nm),
                                                       fptr(em), fptr(yy), int(seed), int(sample_offset), fptr(nz),
                                                       fptr(loss), fptr(pred), fptr(grad), has.ctypes.data_as(_lib.IP)),
                    "gaudi_predictor_loss_grad")
        out, pos = {}, 0
        for name, shape, g in zip(self.pred_names, self.pred_shapes, has):
            size = int(np.prod(shape))
            out[name] = grad[pos:pos + size].reshape(shape) if g else None
            pos += size
        return float(loss[0]), pred, out

    def edm_nll(self, x, onehot, t_int, node_mask, edge_mask, *, seed, sample_offset, noise=None, return_terms=False):
        """The EDM's negative log-likelihood of (x, onehot) in one launch (include/gaudi_hip.h: gaudi_edm_nll) -> nll [B], or
        (nll [B], terms [B,6]) with return_terms: kl_prior, loss_t, neg_log_constants, loss_term_0, delta_log_px, error.
        x [B,N,3] un-normalised, masked, mean-free; onehot [B,N,F]; t_int [B] in 1..T; noise [2,B,N,3+F] raw draws or None
        (Philox draws 0 / 1 of (seed, sample_offset + b))."""
        self._sync_edm()
        x = f32(x)
        B, N = x.shape[0], x.shape[1]
        oh = f32(onehot).reshape(B, N, self.F)
        nm, em = self._masks(f32(node_mask).reshape(B, N), edge_mask, B, N)
        ti = np.ascontiguousarray(np.broadcast_to(np.asarray(t_int).reshape(-1), (B,)), dtype=np.int32)
        nz = None
        if noise is not None:
            nz = f32(noise)
            if nz.shape != (2, B, N, 3 + self.F):
                raise GaudiError(f"noise must be [2,B,N,3+F] = {(2, B, N, 3 + self.F)}, got {nz.shape}")
        nll = np.empty(B, np.float32)
        terms = np.empty((B, 6), np.float32)
        self._check(self.lib.gaudi_edm_nll(self.h, B, N, fptr(x), fptr(oh), ti.ctypes.data_as(_lib.IP), fptr(nm), fptr(em),
                                           int(seed), int(sample_offset), fptr(nz), fptr(nll), fptr(terms)), "gaudi_edm_nll")
        return (nll, terms) if return_terms else nll

    def edm_set_train_weights(self, state_dict: dict):
        """Replace the torch-layout weights the training kernels read (include/gaudi_hip.h: gaudi_edm_set_train_weights) with
        state_dict, in the names, order and shapes given to load_edm.  No repack: the sampler's images go stale, and the next
        sampler-kernel call through this Engine rebuilds them with load_edm first."""
        sd = _strip(state_dict)
        if list(sd.keys()) != self.edm_names:
            raise GaudiError("edm_set_train_weights needs the state dict keys of load_edm, in the same order")
        n, c_names, c_ptrs, c_numel, keep = self._tensor_args(sd)
        self._check(self.lib.gaudi_edm_set_train_weights(self.h, n, c_names, c_ptrs, c_numel), "gaudi_edm_set_train_weights")
        # a copy: _strip may alias the caller's arrays, and the sampler must reload exactly what the training copy holds
        self._edm_train_sd = {k: v.copy() for k, v in sd.items()}

    def edm_loss_grad(self, x, onehot, t_int, node_mask, edge_mask, *, seed=0, sample_offset=0, noise=None, loss_type="l2",
                      weight=None, grad=True):
        """The EDM's train-mode loss per molecule and sum_b weight_b d loss_b / d w (include/gaudi_hip.h: gaudi_edm_loss_grad)
        -> (loss [B], net [B,N,3+F], {name: gradient, or None where the tensor has no gradient path}); with grad=False the
        dict is empty (forward only).  x [B,N,3] un-normalised, masked, mean-free; onehot [B,N,F]; t_int [B] in 0..T;
        noise [B,N,3+F] raw draws or None (Philox draw 0 of (seed, sample_offset + b)); loss_type 'l2' or 'vlb';
        weight [B] or None (1 each)."""
        self._sync_edm(sampler=False)
        if loss_type not in ("l2", "vlb"):
            raise GaudiError(f"diffusion_loss_type must be 'l2' or 'vlb', got {loss_type!r}")
        x = f32(x)
        B, N = x.shape[0], x.shape[1]
        oh = f32(onehot).reshape(B, N, self.F)
        nm, em = self._masks(f32(node_mask).reshape(B, N), edge_mask, B, N)
        ti = np.ascontiguousarray(np.broadcast_to(np.asarray(t_int).reshape(-1), (B,)), dtype=np.int32)
        D = 3 + self.F
        nz = None
        if noise is not None:
            nz = f32(noise)
            if nz.shape != (B, N, D):
                raise GaudiError(f"noise must be [B,N,3+F] = {(B, N, D)}, got {nz.shape}")
        w = None if weight is None else f32(np.broadcast_to(np.asarray(weight, np.float32).reshape(-1), (B,)))
        loss = np.empty(B, np.float32)
        net = np.empty((B, N, D), np.float32)
        gbuf, has = None, None
        if grad:
            n = C.c_int64(0)
            self._check(self.lib.gaudi_edm_grad_size(self.h, C.byref(n)), "gaudi_edm_grad_size")
            gbuf = np.zeros(int(n.value), np.float32)
            has = np.zeros(len(self.edm_names), np.int32)
        self._check(self.lib.gaudi_edm_loss_grad(self.h, B, N, fptr(x), fptr(oh), ti.ctypes.data_as(_lib.IP), fptr(nm),
                                                 fptr(em), int(seed), int(sample_offset), fptr(nz),
                                                 0 if loss_type == "l2" else 1, fptr(w), fptr(loss), fptr(net), fptr(gbuf),
                                                 None if has is None else has.ctypes.data_as(_lib.IP)),
                    "gaudi_edm_loss_grad")
        out = {}
        if grad:
            pos = 0
            for name, shape, g in zip(self.edm_names, self.edm_shapes, has):
                size = int(np.prod(shape))
                out[name] = gbuf[pos:pos + size].reshape(shape) if g else None
                pos += size
        return loss, net, out

    def sample_callback(self, node_mask, edge_mask, target_grad, *, seed=0, sample_offset=0, noise=None, std=1.0,
                        scale=1.0, return_z0=False, with_z=False, grid=None, start=None, return_zt=False):
        """Guided chain for an arbitrary target: ``target_grad(pred [B,K], t) -> dT/dpred [B,K]`` is called once per
        reverse step between the two device phases (include/gaudi_hip.h: gaudi_sample_cb).  with_z=True: the target also
        depends on z outside the predictor -- ``target_grad(z_s [B,N,D], pred [B,K], t) -> (dT/dpred [B,K], dT/dz [B,N,D])``
        with dT/dz the DIRECT part, pred held fixed (gaudi_sample_cbz).  grid / start / return_zt as in sample(): the callback
        then receives t = g[k] / T of the step it belongs to (gaudi_sample_cb_grid)."""
        if grid is None and start is not None:
            raise GaudiError("a start from given molecules needs the time grid to run (grid[0] = the time index to noise to)")
        self._sync_edm()
        self._sync_pred()
        nm = f32(node_mask)
        B, N = nm.shape[0], nm.shape[1]
        nm, em = self._masks(nm, edge_mask, B, N)
        D = 3 + self.F
        nz = None
        if noise is not None:
            nz = f32(noise)
            want = (self.T + 2, 1 if self.fix_noise else B, N, D)
            if nz.shape != want:
                raise GaudiError(f"noise must be [T+2,{'1' if self.fix_noise else 'B'},N,3+F] = {want}, got {nz.shape}")
        x = np.empty((B, N, 3), np.float32)
        h = np.empty((B, N, self.F), np.float32)
        z0 = np.empty((B, N, D), np.float32) if return_z0 else None
        diag = Diag()
        failure = []

        def _cb(_user, b, k, pred_p, t, out_p):
            try:
                pred = np.ctypeslib.as_array(pred_p, shape=(b, k)).copy()
                g = np.ascontiguousarray(target_grad(pred, float(t)), dtype=np.float32)
                if g.shape != (b, k):
                    raise GaudiError(f"target_grad must return [B,K] = {(b, k)}, got {g.shape}")
                np.ctypeslib.as_array(out_p, shape=(b, k))[...] = g
            except BaseException as exc:  # never unwind through the C frames; report after the call returns
                if not failure:
                    failure.append(exc)

        def _cbz(_user, b, n, dd, k, z_p, pred_p, t, out_p, outz_p):
            try:
                zs = np.ctypeslib.as_array(z_p, shape=(b, n, dd)).copy()
                pred = np.ctypeslib.as_array(pred_p, shape=(b, k)).copy()
                g, gz = target_grad(zs, pred, float(t))
                g = np.ascontiguousarray(g, dtype=np.float32)
                gz = np.ascontiguousarray(gz, dtype=np.float32)
                if g.shape != (b, k) or gz.shape != (b, n, dd):
                    raise GaudiError(f"target_grad must return ([B,K], [B,N,D]) = ({(b, k)}, {(b, n, dd)}), got ({g.shape}, {gz.shape})")
                np.ctypeslib.as_array(out_p, shape=(b, k))[...] = g
                np.ctypeslib.as_array(outz_p, shape=(b, n, dd))[...] = gz
            except BaseException as exc:  # never unwind through the C frames; report after the call returns
                if not failure:
                    failure.append(exc)

        zt = None
        what = "gaudi_sample_cbz" if with_z else "gaudi_sample_cb"
        if grid is not None:
            ng, g, x0, oh0, zt = self._grid_args(grid, start, B, N, return_zt)
            cb = TARGET_CBZ(_cbz) if with_z else TARGET_CB(_cb)
            what = "gaudi_sample_cb_grid"
            rc = self.lib.gaudi_sample_cb_grid(self.h, B, N, fptr(nm), fptr(em), int(seed), int(sample_offset), fptr(nz),
                                               float(std), TARGET_CB() if with_z else cb, cb if with_z else TARGET_CBZ(), None,
                                               float(scale), ng, g.ctypes.data_as(_lib.IP), fptr(x0), fptr(oh0), fptr(x), fptr(h),
                                               fptr(z0), fptr(zt), C.byref(diag))
        elif with_z:
            cb = TARGET_CBZ(_cbz)
            rc = self.lib.gaudi_sample_cbz(self.h, B, N, fptr(nm), fptr(em), int(seed), int(sample_offset), fptr(nz),
                                           float(std), cb, None, float(scale), fptr(x), fptr(h), fptr(z0), C.byref(diag))
        else:
            cb = TARGET_CB(_cb)
            rc = self.lib.gaudi_sample_cb(self.h, B, N, fptr(nm), fptr(em), int(seed), int(sample_offset), fptr(nz),
                                          float(std), cb, None, float(scale), fptr(x), fptr(h), fptr(z0), C.byref(diag))
        if failure:
            raise failure[0]
        self._check(rc, what)
        d = dict(max_masked_leak=diag.max_masked_leak, max_cog_rel=diag.max_cog_rel, max_cog_abs=diag.max_cog_abs,
                 nan_count=diag.nan_count, reprojected=diag.reprojected,
                 edge_math_fallback=getattr(self, "_fallback_reason", None), family_split_resident=self.family_split())
        out = (x, h, d) + ((z0,) if return_z0 else ())
        return out + (zt,) if return_zt else out

    # ------------------------------------------------------------------ fused value targets
    def sample_target(self, node_mask, edge_mask, spec, *, seed=0, sample_offset=0, noise=None, std=1.0, grid=None, start=None,
                      return_z0=False, return_zt=False, trace=False):
        """Guided chain for the fused value-target family (include/gaudi_hip.h: gaudi_sample_target) -> (x, h, diag[, z0][, zt]
        [, trace]).  spec: dict with any of w, q, c, side ([K] shared or [B,K] per molecule), scale (float or [B]) and
        window = (t_lo, t_hi) in time indices (see target_spec).  trace=True also returns [steps, B, K+2]: the predictions at
        every guided step, the gradient's 2-norm before the clip and the clip coefficient (zero rows outside the window).
        grid / start / return_zt as in sample()."""
        if grid is None and start is not None:
            raise GaudiError("a start from given molecules needs the time grid to run (grid[0] = the time index to noise to)")
        self._sync_edm()
        self._sync_pred()
        nm = f32(node_mask)
        B, N = nm.shape[0], nm.shape[1]
        nm, em = self._masks(nm, edge_mask, B, N)
        D = 3 + self.F
        nz = None
        if noise is not None:
            nz = f32(noise)
            want = (self.T + 2, 1 if self.fix_noise else B, N, D)
            if nz.shape != want:
                raise GaudiError(f"noise must be [T+2,{'1' if self.fix_noise else 'B'},N,3+F] = {want}, got {nz.shape}")
        cs, keep = target_spec(spec, B, self.K)
        x = np.empty((B, N, 3), np.float32)
        h = np.empty((B, N, self.F), np.float32)
        z0 = np.empty((B, N, D), np.float32) if return_z0 else None
        diag = Diag()
        ng, g, x0, oh0, zt = 0, None, None, None, None
        if grid is not None:
            ng, g, x0, oh0, zt = self._grid_args(grid, start, B, N, return_zt)
        elif return_zt:
            raise GaudiError("return_zt needs a start from given molecules (start=(x, onehot))")
        steps = self.T if grid is None else ng - 1
        tr = np.zeros((max(steps, 0), B, self.K + 2), np.float32) if trace else None
        self._check(self.lib.gaudi_sample_target(self.h, B, N, fptr(nm), fptr(em), int(seed), int(sample_offset), fptr(nz),
                                                 float(std), C.byref(cs), ng, None if g is None else g.ctypes.data_as(_lib.IP),
                                                 fptr(x0), fptr(oh0), fptr(x), fptr(h), fptr(z0), fptr(zt), fptr(tr),
                                                 C.byref(diag)), "gaudi_sample_target")
        del keep
        d = dict(max_masked_leak=diag.max_masked_leak, max_cog_rel=diag.max_cog_rel, max_cog_abs=diag.max_cog_abs,
                 nan_count=diag.nan_count, reprojected=diag.reprojected,
                 edge_math_fallback=getattr(self, "_fallback_reason", None), family_split_resident=self.family_split())
        out = (x, h, d) + ((z0,) if return_z0 else ()) + ((zt,) if return_zt else ())
        return out + (tr,) if trace else out

    def step_target(self, s_idx, z_t, node_mask, edge_mask, eps_raw, spec, *, t_idx=None, trace=False):
        """One teacher-forced guided step z_t -> z_s (time index t_idx, default s_idx + 1, down to s_idx) for a value-target
        spec (gaudi_step_target) -> z_s, or (z_s, trace row [B, K+2]) with trace=True."""
        self._sync_edm()
        self._sync_pred()
        z = f32(z_t)
        B, N, D = z.shape
        nm, em = self._masks(node_mask, edge_mask, B, N)
        eps = f32(eps_raw)
        cs, keep = target_spec(spec, B, self.K)
        out = np.empty_like(z)
        tr = np.zeros((B, self.K + 2), np.float32) if trace else None
        self._check(self.lib.gaudi_step_target(self.h, B, N, int(s_idx), int(s_idx) + 1 if t_idx is None else int(t_idx), fptr(z),
                                               fptr(nm), fptr(em), fptr(eps), C.byref(cs), fptr(out), fptr(tr)),
                    "gaudi_step_target")
        del keep
        return (out, tr) if trace else out

    def sample_chain(self, node_mask, edge_mask, keep_frames, *, seed=0, sample_offset=0, noise=None, std=1.0):
        """-> chain [keep_frames, B, N, 3+F] (frame 0 = final [x | one_hot]).  Unit time grid only: the reference's frame rule
        (frame (s * keep_frames) // T) is defined on it, so this call takes no grid."""
        self._sync_edm()
        self._sync_pred()
        nm = f32(node_mask)
        B, N = nm.shape[0], nm.shape[1]
        nm, em = self._masks(nm, edge_mask, B, N)
        D = 3 + self.F
        nz = None if noise is None else f32(noise)
        chain = np.empty((int(keep_frames), B, N, D), np.float32)
        self._check(self.lib.gaudi_sample_chain(self.h, B, N, fptr(nm), fptr(em), int(seed), int(sample_offset), fptr(nz),
                                                float(std), int(keep_frames), fptr(chain)), "gaudi_sample_chain")
        return chain

    def philox_normal(self, seed, sample_offset, B, n_elem, draw0, n_draws) -> np.ndarray:
        out = np.empty((n_draws, B, n_elem), np.float32)
        self._check(self.lib.gaudi_philox_normal(self.h, int(seed), int(sample_offset), B, n_elem, draw0, n_draws,
                                                 fptr(out)), "gaudi_philox_normal")
        return out

    # ------------------------------------------------------------------ profiling
    def profile_reset(self, enable=True):
        self._check(self.lib.gaudi_profile_reset(self.h, int(enable)), "gaudi_profile_reset")

    def profile_get(self):
        n = C.c_int32()
        ms = C.c_double()
        steps = C.c_int64()
        self._check(self.lib.gaudi_profile_get(self.h, C.byref(n), C.byref(ms), C.byref(steps)), "gaudi_profile_get")
        return n.value, ms.value, steps.value

    def stability_profile_get(self):
        n = C.c_int32()
        ms = C.c_double()
        self._check(self.lib.gaudi_stability_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_stability_profile_get")
        return n.value, ms.value

    def atoms_profile_get(self):
        """(launches, summed milliseconds) of gaudi_rings_to_atoms since profile_reset(True)."""
        n = C.c_int32()
        ms = C.c_double()
        self._check(self.lib.gaudi_atoms_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_atoms_profile_get")
        return n.value, ms.value

    def rings_to_atoms(self, tables, atom_tables, x, ring_type, n_nodes, flags, max_atoms, max_bonds):
        """gaudi_rings_to_atoms on packed arrays (x [B,N,3] float32, ring_type [B,N] int32, n_nodes [B] int32) -> dict of the
        raw output arrays; gaudi_amd.gor2goa.rings_to_atoms is the interface on top."""
        B, N = x.shape[0], x.shape[1]
        out = dict(n_atoms=np.zeros(B, np.int32), atom_type=np.zeros((B, max_atoms), np.int32),
                   xy=np.zeros((B, max_atoms, 2), np.float64), xyz=np.zeros((B, max_atoms, 3), np.float64),
                   n_bonds=np.zeros(B, np.int32), bonds=np.zeros((B, max_bonds, 2), np.int32), status=np.zeros(B, np.int32),
                   fingerprint=np.zeros(B, np.uint64))
        ip = lambda a: a.ctypes.data_as(_lib.IP)
        dp = lambda a: a.ctypes.data_as(_lib.DP)
        rc = self.lib.gaudi_rings_to_atoms(self.h, C.byref(tables), C.byref(atom_tables), B, N, fptr(x), ip(ring_type), ip(n_nodes),
                                           int(flags), int(max_atoms), int(max_bonds), ip(out["n_atoms"]), ip(out["atom_type"]),
                                           dp(out["xy"]), dp(out["xyz"]), ip(out["n_bonds"]), ip(out["bonds"]), ip(out["status"]),
                                           out["fingerprint"].ctypes.data_as(C.POINTER(C.c_uint64)))
        self._check(rc, "gaudi_rings_to_atoms")
        return out

    def rings_profile_get(self):
        """(launches, summed milliseconds) of gaudi_atoms_to_rings since profile_reset(True)."""
        n = C.c_int32()
        ms = C.c_double()
        self._check(self.lib.gaudi_rings_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_rings_profile_get")
        return n.value, ms.value

    def atoms_to_rings(self, tables, xyz, elem, n_atoms, flags=0, covalency_factor=1.3, max_rings=_lib.RINGS_MAX_RINGS):
        """gaudi_atoms_to_rings on packed arrays (xyz [B,A,3] float64, elem [B,A] int32, n_atoms [B] int32) -> dict of the raw
        output arrays; gaudi_amd.goa2gor.atoms_to_rings is the interface on top."""
        out = _lib.rings_outputs(xyz.shape[0], max_rings)
        rc = self.lib.gaudi_atoms_to_rings(self.h, C.byref(tables), *_lib.rings_args(xyz, elem, n_atoms, flags, covalency_factor,
                                                                                     max_rings, out))
        self._check(rc, "gaudi_atoms_to_rings")
        return out

    def bonds_profile_get(self):
        """(launches, summed milliseconds) of gaudi_bond_orders since profile_reset(True)."""
        n = C.c_int32()
        ms = C.c_double()
        self._check(self.lib.gaudi_bonds_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_bonds_profile_get")
        return n.value, ms.value

    def bond_orders(self, tables, elem, n_atoms, bonds, n_bonds):
        """gaudi_bond_orders on packed arrays (elem [B,A], n_atoms [B], bonds [B,M,2], n_bonds [B], all int32) -> dict of the raw
        output arrays (order [B,M] uint8, charge [B,A] int8, n_charged [B], status [B]); gaudi_amd.gor2goa.bond_orders is the
        interface on top."""
        out = _lib.bonds_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        rc = self.lib.gaudi_bond_orders(self.h, C.byref(tables), *_lib.bonds_args(elem, n_atoms, bonds, n_bonds, out))
        self._check(rc, "gaudi_bond_orders")
        return out

    def kekule_profile_get(self):
        """(launches, summed milliseconds) of gaudi_kekule since profile_reset(True)."""
        n = C.c_int32()
        ms = C.c_double()
        self._check(self.lib.gaudi_kekule_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_kekule_profile_get")
        return n.value, ms.value

    def kekule(self, tables, elem, n_atoms, bonds, n_bonds):
        """gaudi_kekule on packed arrays (as bond_orders takes them) -> dict of the raw output arrays (_lib.KEKULE_ARRAYS: k [B]
        int64, double_count [B,M] uint32, n_hex [B], hex_atoms [B,32,6] int32, sextet_count [B,32] uint32, fries / clar [B],
        n_nodes [B] int64, status [B]); gaudi_amd.aromaticity.resonance is the interface on top."""
        out = _lib.kekule_outputs(elem.shape[0], bonds.shape[1])
        rc = self.lib.gaudi_kekule(self.h, C.byref(tables), *_lib.kekule_args(elem, n_atoms, bonds, n_bonds, out))
        self._check(rc, "gaudi_kekule")
        return out

    def canon_profile_get(self):
        """(launches, summed milliseconds) of gaudi_canonical_order since profile_reset(True)."""
        n = C.c_int32()
        ms = C.c_double()
        self._check(self.lib.gaudi_canon_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_canon_profile_get")
        return n.value, ms.value

    def canonical_order(self, n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds):
        """gaudi_canonical_order on packed arrays (as bond_orders takes them) -> dict of the raw output arrays (rank [B,A] int32,
        n_heavy [B], label [B,A] uint8, n_hbonds [B], cbonds [B,M,2] uint16, nodes [B], status [B]);
        gaudi_amd.gor2goa.canonical is the interface on top."""
        out = _lib.canon_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        rc = self.lib.gaudi_canonical_order(self.h, *_lib.canon_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, out))
        self._check(rc, "gaudi_canonical_order")
        return out

    def fp_profile_get(self):
        """(calls, summed milliseconds of their kernels) of the fingerprint / nearest / common calls since profile_reset(True)."""
        n = C.c_int32()
        ms = C.c_double()
        self._check(self.lib.gaudi_fp_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_fp_profile_get")
        return n.value, ms.value

    def circular_fingerprint(self, n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, radius=2, n_bins=1024):
        """gaudi_circular_fingerprint on packed arrays (as bond_orders takes them) -> dict of the raw output arrays (fp [B,n_bins]
        uint8, total [B], status [B]); gaudi_amd.similarity.fingerprints is the interface on top."""
        if n_bins not in _lib.FP_BINS:
            raise GaudiError(f"n_bins must be one of {_lib.FP_BINS}, got {n_bins}")
        out = _lib.fp_outputs(elem.shape[0], n_bins)
        rc = self.lib.gaudi_circular_fingerprint(self.h, *_lib.fp_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, radius,
                                                                       n_bins, out))
        self._check(rc, "gaudi_circular_fingerprint")
        return out

    def substructure_profile_get(self):
        """(launches, summed milliseconds) of gaudi_substructure_search since profile_reset(True)."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_substructure_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_substructure_profile_get")
        return int(n.value), float(ms.value)

    def substructure_search(self, n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, p_elem, p_n_atoms, p_bonds, p_n_bonds,
                            p_flags):
        """gaudi_substructure_search on packed arrays: the molecules as bond_orders takes them, at most 64 patterns in the same
        layout and their flags -> dict of the raw output arrays (count [B,P] int32, first [B,P,QA] int32, covered [B,P,A] uint8,
        steps [B,P] int32, status [B,P] int32).  gaudi_amd.substructure.search is the interface on top."""
        out = _lib.sub_outputs(elem.shape[0], p_elem.shape[0], elem.shape[1], p_elem.shape[1])
        rc = self.lib.gaudi_substructure_search(self.h, *_lib.sub_args(n_elems, h_elem, c_elem, elem, n_atoms, bonds, n_bonds, p_elem,
                                                                       p_n_atoms, p_bonds, p_n_bonds, p_flags, out))
        self._check(rc, "gaudi_substructure_search")
        return out

    def huckel_profile_get(self):
        """(launches, summed milliseconds) of gaudi_huckel since profile_reset(True): one launch per capacity tier present."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_huckel_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_huckel_profile_get")
        return int(n.value), float(ms.value)

    def huckel(self, tables, elem, n_atoms, bonds, n_bonds, charge=None):
        """gaudi_huckel on packed arrays: a HuckelTables (gaudi_amd.huckel.c_huckel_tables), the molecules as bond_orders takes
        them, charge [B] int32 or None -> dict of the raw output arrays (_lib.HUCKEL_ARRAYS: levels [B,128] float32, occupation
        [B,128] uint8, n_pi / n_electrons / n_excluded / sweeps / flags / status [B] int32, homo / lumo / gap / e_pi [B] float32,
        pi_charge [B,A] float32, pi_bond_order [B,M] float32, site_class [B,A] int8).  gaudi_amd.huckel.orbitals is the interface
        on top."""
        out = _lib.huckel_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        rc = self.lib.gaudi_huckel(self.h, *_lib.huckel_args(tables, elem, n_atoms, bonds, n_bonds, charge, out))
        self._check(rc, "gaudi_huckel")
        return out

    def ppp_profile_get(self):
        """(launches, summed milliseconds) of gaudi_ppp since profile_reset(True): one launch per capacity tier present."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_ppp_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_ppp_profile_get")
        return int(n.value), float(ms.value)

    def ppp(self, tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, repulsion=0, damping=0.25):
        """gaudi_ppp on packed arrays: a PPPTables (gaudi_amd.ppp.c_ppp_tables), the molecules as bond_orders takes them, xyz
        [B,A,3] float32 in Angstrom, charge [B] int32 or None, the repulsion formula (0 Mataga-Nishimoto, 1 Ohno) and the damping
        -> dict of the raw output arrays (_lib.PPP_ARRAYS: levels [B,128] float32 in eV, occupation [B,128] uint8, pi_charge [B,A],
        pi_bond_order [B,M] float32, site_class [B,A] int8, n_pi / n_electrons / n_excluded / iterations / sweeps / flags / status
        [B] int32, homo / lumo / gap / e_electronic / e_core / delta_p [B] float32).  gaudi_amd.ppp.orbitals is the interface on
        top."""
        out = _lib.ppp_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        rc = self.lib.gaudi_ppp(self.h, *_lib.ppp_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, repulsion, damping, out))
        self._check(rc, "gaudi_ppp")
        return out

    def ppp_open_profile_get(self):
        """(launches, summed milliseconds) of gaudi_ppp_open since profile_reset(True): one launch per capacity tier present."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_ppp_open_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_ppp_open_profile_get")
        return int(n.value), float(ms.value)

    def ppp_open(self, tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, multiplicity=None, repulsion=0, damping=0.25):
        """gaudi_ppp_open on packed arrays: ``ppp``'s arguments with multiplicity [B] int32 or None (0: the lowest the parity
        allows) behind the charge -> dict of ``ppp``'s eighteen arrays (occupation 2 / 1 / 0) and spin_density [B,A] float32,
        e_state / he_correction [B] float64, n_open [B] and somo [B,2] int32 (_lib.PPP_OPEN_ARRAYS).  gaudi_amd.ppp.states is
        the interface on top."""
        out = _lib.ppp_open_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        rc = self.lib.gaudi_ppp_open(self.h, *_lib.ppp_open_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity,
                                                                 repulsion, damping, out))
        self._check(rc, "gaudi_ppp_open")
        return out

    def ppp_scf_profile_get(self):
        """(launches, summed milliseconds) of gaudi_ppp_scf since profile_reset(True): one launch per capacity tier present, more
        where a tier's scratch is split."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_ppp_scf_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_ppp_scf_profile_get")
        return int(n.value), float(ms.value)

    def ppp_scf(self, tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, multiplicity=None, repulsion=0, diis_size=6, diis_start=3,
                damping=0.25):
        """gaudi_ppp_scf on packed arrays: ``ppp_open``'s arguments with the DIIS history's length (2..8) and its first iteration
        (at least 2) in front of the damping -> dict of ``ppp_open``'s twenty-three arrays and diis_error [B] float32, n_extrapolated
        [B] int32 (_lib.PPP_SCF_ARRAYS).  gaudi_amd.ppp.states(..., scf="diis") is the interface on top."""
        out = _lib.ppp_scf_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        rc = self.lib.gaudi_ppp_scf(self.h, *_lib.ppp_scf_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, multiplicity,
                                                               repulsion, diis_size, diis_start, damping, out))
        self._check(rc, "gaudi_ppp_scf")
        return out

    def ring_currents_profile_get(self):
        """(launches, summed milliseconds) of gaudi_ring_currents since profile_reset(True): one launch per capacity tier present."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_ring_currents_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_ring_currents_profile_get")
        return int(n.value), float(ms.value)

    def ring_currents(self, tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None):
        """gaudi_ring_currents on packed arrays: a HuckelTables (gaudi_amd.huckel.c_huckel_tables), the molecules as bond_orders
        takes them, xyz [B,A,3] float32 in Angstrom, charge [B] int32 or None -> dict of the raw output arrays
        (_lib.RING_CURRENT_ARRAYS: bond_current [B,M] float32, n_rings [B], ring_atoms [B,32,6], ring_size [B,32] int32, ring_current /
        ring_area [B,32], normal [B,3], rms_out_of_plane / gap / residual [B] float32, n_pi / n_electrons / sweeps / flags / status [B]
        int32).  gaudi_amd.aromaticity.ring_currents is the interface on top."""
        out = _lib.ring_current_outputs(elem.shape[0], bonds.shape[1])
        rc = self.lib.gaudi_ring_currents(self.h, *_lib.ring_current_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, out))
        self._check(rc, "gaudi_ring_currents")
        return out

    def reactivity_profile_get(self):
        """(launches, summed milliseconds) of gaudi_reactivity since profile_reset(True): one launch per capacity tier present."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_reactivity_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_reactivity_profile_get")
        return int(n.value), float(ms.value)

    def reactivity(self, tables, elem, n_atoms, bonds, n_bonds, charge=None, with_bonds=True, slices=0):
        """gaudi_reactivity on packed arrays: a HuckelTables (gaudi_amd.huckel.c_huckel_tables), the molecules as bond_orders takes
        them, charge [B] int32 or None, with_bonds (the ortho localization energies: one more solve per pi bond), slices (waves
        per molecule, 1..16; 0: chosen from the compute units and the batch) -> dict of the raw output arrays
        (_lib.REACTIVITY_ARRAYS: atom_localization [B,3,A], free_valence [B,A] float32, rings [B,32,6], n_rings [B] int32,
        para_localization [B,32,3], ortho_localization [B,M], e_pi [B] float32, n_pi / n_electrons / n_jobs / sweeps / flags /
        status [B] int32; NaN where an entry does not apply).  gaudi_amd.reactivity.localization is the interface on top."""
        out = _lib.reactivity_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        rc = self.lib.gaudi_reactivity(self.h, *_lib.reactivity_args(tables, elem, n_atoms, bonds, n_bonds, charge, with_bonds, slices, out))
        self._check(rc, "gaudi_reactivity")
        return out

    def ppp_cis_profile_get(self):
        """(launches, summed milliseconds) of the CIS kernel of gaudi_ppp_cis since profile_reset(True): one launch per call (the
        SCF launches of those calls are ppp_profile_get's)."""
        n, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gaudi_ppp_cis_profile_get(self.h, C.byref(n), C.byref(ms)), "gaudi_ppp_cis_profile_get")
        return int(n.value), float(ms.value)

    def ppp_cis(self, tables, elem, n_atoms, bonds, n_bonds, xyz, charge=None, repulsion=0, damping=0.25, window=8):
        """gaudi_ppp_cis on packed arrays: ``ppp``'s arguments and the active window (1..8) -> dict of ``ppp``'s eighteen arrays
        (flags with the CIS bits) and _lib.PPP_CIS_ARRAYS: singlet / triplet / osc / lead_weight [B,64] float32, dipole [B,64,3]
        float32, lead [B,64,2] uint8, n_states / n_active_occ / n_active_virt / cis_sweeps [B] int32.
        gaudi_amd.ppp.excited_states is the interface on top."""
        out = _lib.ppp_outputs(elem.shape[0], elem.shape[1], bonds.shape[1])
        out.update(_lib.ppp_cis_outputs(elem.shape[0]))
        rc = self.lib.gaudi_ppp_cis(self.h, *(_lib.ppp_args(tables, elem, n_atoms, bonds, n_bonds, xyz, charge, repulsion, damping, out)
                                              + _lib.ppp_cis_args(window, out)))
        self._check(rc, "gaudi_ppp_cis")
        return out

    def fp_library_set(self, fp=None):
        """gaudi_fp_library_set: keep fp [M,n_bins] uint8 on the device as THE resident library of this engine (None: free it)."""
        if fp is None:
            self._check(self.lib.gaudi_fp_library_set(self.h, 0, 0, None), "gaudi_fp_library_set")
            return
        fp = _lib.fp_rows(fp)
        self._check(self.lib.gaudi_fp_library_set(self.h, fp.shape[1], fp.shape[0], fp.ctypes.data_as(_lib.U8P)), "gaudi_fp_library_set")

    def fp_nearest(self, q, lib=None, k=1, M=None):
        """gaudi_fp_nearest: q [B,n_bins] against lib [M,n_bins], or against the resident library of M rows when lib is None ->
        dict(idx, common, union), each int32 [B,k]."""
        q = _lib.fp_rows(q)
        lib = None if lib is None else _lib.fp_rows(lib)
        out = _lib.nearest_outputs(q.shape[0], k)
        rc = self.lib.gaudi_fp_nearest(self.h, q.shape[1], q.shape[0], q.ctypes.data_as(_lib.U8P), int(M if lib is None else lib.shape[0]),
                                       None if lib is None else lib.ctypes.data_as(_lib.U8P), int(k),
                                       *(out[n].ctypes.data_as(_lib.IP) for n in ("idx", "common", "union")))
        self._check(rc, "gaudi_fp_nearest")
        return out

    def fp_common(self, q, lib=None, M=None):
        """gaudi_fp_common: the sum of the byte-wise minimum for every pair -> int32 [B,M]."""
        q = _lib.fp_rows(q)
        lib = None if lib is None else _lib.fp_rows(lib)
        M = int(M if lib is None else lib.shape[0])
        out = np.zeros((q.shape[0], max(M, 0)), np.int32)
        rc = self.lib.gaudi_fp_common(self.h, q.shape[1], q.shape[0], q.ctypes.data_as(_lib.U8P), M,
                                      None if lib is None else lib.ctypes.data_as(_lib.U8P), out.ctypes.data_as(_lib.IP))
        self._check(rc, "gaudi_fp_common")
        return out

    def fp_neighbours(self, rows, num, den):
        """gaudi_fp_neighbours: for every row of rows [N,n_bins] the live rows at least num / den similar to it, itself included ->
        dict(count int32 [N], offsets int64 [N+1], list int32 [offsets[N]]: ascending, CSR)."""
        return _lib.fp_neighbours_call(self.lib.gaudi_fp_neighbours, (self.h,), rows, num, den, self._check)

    def fp_cluster(self, rows, num, den):
        """gaudi_fp_cluster: Butina clusters at num / den -> dict(cluster, centroid, size, count: int32 [N]; n_clusters)."""
        return _lib.fp_cluster_call(self.lib.gaudi_fp_cluster, (self.h,), rows, num, den, self._check)

    def fp_pick_diverse(self, rows, k, num=0, den=0, seeds=None, first=-1, S=None):
        """gaudi_fp_pick_diverse: up to k MaxMin picks from rows [N,n_bins].  seeds [S,n_bins], or None with S > 0 for the resident
        library of S rows; den = 0: no threshold -> dict(picked, pick_common, pick_union: int32 [k]; n_picked; owner, owner_common,
        owner_union: int32 [N])."""
        S = (0 if seeds is None else len(seeds)) if S is None else int(S)
        return _lib.fp_pick_call(self.lib.gaudi_fp_pick_diverse, (self.h,), rows, S, seeds, first, k, num, den, self._check)

    FP_SELECT_STAGES = ("count", "offsets", "fill", "sort", "walk", "pick_setup", "pick_rounds", "totals")

    def fp_select_stages_get(self) -> dict:
        """gaudi_fp_select_stages_get: the kernel milliseconds, by stage, of the most recent fp_neighbours / fp_cluster /
        fp_pick_diverse call made after profile_reset(True); a stage the call did not run is 0.0."""
        ms = np.zeros(len(self.FP_SELECT_STAGES), np.float64)
        self._check(self.lib.gaudi_fp_select_stages_get(self.h, ms.ctypes.data_as(_lib.DP)), "gaudi_fp_select_stages_get")
        return dict(zip(self.FP_SELECT_STAGES, ms.tolist()))

    def set_fix_noise(self, enable: bool, key_sample: int = 0):
        """fix_noise=True of the reference (en_diffusion.py:562-566): every molecule of a call receives the raw draws of
        ONE sample (Philox stream of global sample ``key_sample``, or injected noise of shape [T+2,1,N,3+F])."""
        self._check(self.lib.gaudi_set_fix_noise(self.h, int(bool(enable)), int(key_sample)), "gaudi_set_fix_noise")
        self.fix_noise = bool(enable)

    def kernel_variant(self):
        """-> (configured, last_call): 8 = eight waves per molecule (default), 4 = four waves (GAUDI_WAVES=4 or fallback)."""
        a, b = C.c_int32(), C.c_int32()
        self._check(self.lib.gaudi_kernel_variant(self.h, C.byref(a), C.byref(b)), "gaudi_kernel_variant")
        return a.value, b.value

    def edge_math(self):
        """-> (configured, last_call): 1 = edge GEMMs on the bf16 matrix pipe with exactly split fp32 operands (default on the
        8-wave kernels; last_call 2 = the same with the half-size LDS weight ring), 0 = fp32 matrix instructions
        (GAUDI_EDGE_MATH=fp32, the 4-wave kernels, or the LDS fallback)."""
        a, b = C.c_int32(), C.c_int32()
        self._check(self.lib.gaudi_edge_math(self.h, C.byref(a), C.byref(b)), "gaudi_edge_math")
        return a.value, b.value

    def node_buffers_global(self) -> bool:
        """True if the most recent call kept its node buffers in a global scratch (molecules beyond the LDS limit: the V8G kernels
        on 8 waves, the V4G kernels on 4 -- kernel_variant() tells which)."""
        v = C.c_int32()
        self._check(self.lib.gaudi_node_buffers(self.h, C.byref(v)), "gaudi_node_buffers")
        return v.value in (1, 2)

    def node_buffers_form(self) -> int:
        """0: the most recent call kept its node buffers in LDS; 1: in a global scratch; 2: in a global scratch except P and Q, which
        stayed in LDS (8-wave kernels, round 6: kern8gp_*.hip -- taken where that plan fits); 3: in LDS except ONE of the predictor's
        five (wide groups on the full weight ring, round 6: kern8mp_fused.hip)."""
        v = C.c_int32()
        self._check(self.lib.gaudi_node_buffers(self.h, C.byref(v)), "gaudi_node_buffers")
        return int(v.value)

    def last_workgroups(self) -> int:
        """Workgroups of the most recent launch (molecules, or the groups they were packed into)."""
        return self.last_launch_shape()[0]

    def last_launch_shape(self):
        """-> (workgroups, node slots per workgroup) of the most recent launch; node slots > N: wide groups."""
        n, ns = C.c_int32(), C.c_int32()
        self._check(self.lib.gaudi_last_workgroups(self.h, C.byref(n), C.byref(ns)), "gaudi_last_workgroups")
        return n.value, ns.value

    def set_plan_hint(self, min_slots: int = 0, force_waves: int = 0):
        """Plan the following calls with the graph figures of a larger logical batch (see gaudi_set_plan_hint)."""
        self._check(self.lib.gaudi_set_plan_hint(self.h, int(min_slots), int(force_waves)), "gaudi_set_plan_hint")
        self._plan_hint = (int(min_slots), int(force_waves))

    def plan_hint_for(self, node_mask, edge_mask):
        """(min_slots, force_waves) of a WHOLE logical batch: what every shard of it passes to set_plan_hint so that all
        shards run the same kernel family and edge-GEMM arithmetic (device-free: gaudi_host_graph_meta8)."""
        nm = f32(node_mask)
        B, N = nm.shape[0], nm.shape[1]
        nm, em = self._masks(nm, edge_mask, B, N)
        slots = C.c_int32()
        rc = self.lib.gaudi_host_graph_meta8(B, N, fptr(nm), fptr(em), C.byref(slots), None, None, None, None, None, None,
                                             None, 0, None)
        if rc == -5:  # GAUDI_E_CAPACITY: a node with more than 32 live edges -> the 4-wave kernels for everybody
            return 0, 4
        if rc != 0:
            raise GaudiError(f"gaudi_host_graph_meta8 failed ({rc})")
        return int(slots.value), 0

    def pack_plan(self, node_mask, edge_mask, node_slots=None, tiles=16):
        """-> (G, group_of[B], ntiles[G], ncols[G]): the workgroups a sampling call of the 8-wave kernels launches for this
        batch -- small molecules share a workgroup as components of one disjoint graph (device-free: gaudi_host_pack_plan;
        G = B when nothing packs).  node_slots > N: the plan of WIDE groups (gaudi_host_pack_plan_wide)."""
        nm = f32(node_mask)
        B, N = nm.shape[0], nm.shape[1]
        nm, em = self._masks(nm, edge_mask, B, N)
        G = C.c_int32()
        group_of, ntiles, ncols = (np.zeros(B, np.int32) for _ in range(3))
        i32 = C.POINTER(C.c_int32)
        if node_slots is not None and node_slots > N:
            rc = self.lib.gaudi_host_pack_plan_wide(B, N, int(node_slots), int(tiles), fptr(nm), fptr(em), C.byref(G),
                                                    group_of.ctypes.data_as(i32), ntiles.ctypes.data_as(i32), ncols.ctypes.data_as(i32))
        else:
            rc = self.lib.gaudi_host_pack_plan(B, N, fptr(nm), fptr(em), C.byref(G), group_of.ctypes.data_as(i32),
                                               ntiles.ctypes.data_as(i32), ncols.ctypes.data_as(i32))
        if rc != 0:
            raise GaudiError(f"gaudi_host_pack_plan failed ({rc})")
        return G.value, group_of, ntiles[:G.value], ncols[:G.value]

    def set_steps_per_launch(self, k: int):
        self._check(self.lib.gaudi_set_steps_per_launch(self.h, int(k)), "gaudi_set_steps_per_launch")
