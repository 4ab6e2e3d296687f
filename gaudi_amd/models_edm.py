"""Host mirror of models_edm.get_model / EnVariationalDiffusion's sampling interface
(models_edm.py:61-104, edm/equivariant_diffusion/en_diffusion.py:958-1067), backed by libgaudi_hip.so."""
from __future__ import annotations

import numpy as np

from . import checkpoint
from ._lib import GaudiError
from .engine import Engine


def _to_numpy(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _like_ref(a):
    """The reference returns torch tensors; do the same when torch is importable."""
    try:
        import torch
        return torch.from_numpy(np.ascontiguousarray(a))
    except Exception:  # pragma: no cover
        return a


class DistributionRings:
    """models_edm.DistributionRings (models_edm.py:21-58): ring-count sampler over the dataset histogram
    (utils/helpers.py:64-95; shipped as data in gaudi_amd/data/ring_tables.json, histogram order preserved).
    sample() draws through torch.distributions.Categorical exactly as the reference does, so a run seeded with
    torch.manual_seed reproduces the reference's ring counts."""

    def __init__(self, dataset="cata"):
        import torch
        from torch.distributions.categorical import Categorical

        from .analyze import ring_tables
        hist = ring_tables()["n_nodes"]["cata" if dataset == "peri" else dataset]
        self.n_nodes = torch.tensor([int(k) for k in hist])
        self.keys = {int(k): i for i, k in enumerate(hist)}
        prob = np.array([hist[k] for k in hist])
        prob = prob / np.sum(prob)
        self.prob = torch.from_numpy(prob).float()
        self.m = Categorical(torch.tensor(prob))

    def sample(self, n_samples=1):
        return self.n_nodes[self.m.sample((n_samples,))]

    def log_prob(self, batch_n_nodes):
        import torch
        assert len(batch_n_nodes.size()) == 1
        idcs = torch.tensor([self.keys[i.item()] for i in batch_n_nodes])
        return torch.log(self.prob + 1e-30)[idcs]


class PropertyNorm:
    """DistributionProperty(only_norm=True): mean/std + (un)normalize (models_edm.py:107-113,186-192).
    mean/std are NOT stored in checkpoints (they come from the dataset) and must be supplied."""

    def __init__(self, mean, std):
        self.mean = np.asarray(_to_numpy(mean), np.float32)
        self.std = np.asarray(_to_numpy(std), np.float32)

    def _ms(self, like):
        """mean / std in the type of ``like``: the reference's DistributionProperty holds torch tensors, and a target closure
        calls prop_dist.unnormalize on a torch prediction that requires grad (generation_guidance.py:205-211)."""
        if hasattr(like, "detach"):
            import torch
            return (torch.as_tensor(self.mean, dtype=like.dtype, device=like.device),
                    torch.as_tensor(self.std, dtype=like.dtype, device=like.device))
        return self.mean, self.std

    def normalize(self, pred):
        mean, std = self._ms(pred)
        return (pred - mean) / std

    def unnormalize(self, pred):
        mean, std = self._ms(pred)
        return pred * std + mean


class LinearTarget:
    """Declarative target function T(pred) = w . pred + c of the predictor outputs -- the native form of the
    closures in generation_guidance.py:198-211.  Calling it evaluates T on the GPU (predictor forward)."""

    def __init__(self, cond_predictor, weights, const=0.0, name="linear"):
        self.cond_predictor = cond_predictor
        self.weights = np.asarray(weights, np.float32)
        self.const = float(const)
        self.name = name

    def __call__(self, _input, _node_mask, _edge_mask, _t):
        pred = _to_numpy(self.cond_predictor(_input, _node_mask, _edge_mask, _t))
        return _like_ref((pred @ self.weights + self.const).astype(np.float32))


class ValueTarget:
    """Declarative value-seeking target of the predictor outputs, per molecule b:
        T_b(p) = sum_k w[b,k] p[k] + sum_k q[b,k] a(p[k] - c[b,k], side[b,k])^2
    with a(d, 0) = d (aim at the value c), a(d, +1) = max(d, 0) (c is an upper bound), a(d, -1) = min(d, 0) (c is a lower
    bound).  weights / curvature / center / side are [K] (shared) or [B,K] (one row per molecule of the call), scale a float
    or [B] (the call's own ``scale`` argument multiplies it), window = (t_lo, t_hi): only steps starting at time indices
    t_lo..t_hi are guided.  Runs fused on the device (gaudi_sample_target): no per-step callback.  Calling it with the
    reference's closure signature evaluates T on the GPU predictor's output (design() / get_target_function_values)."""

    def __init__(self, cond_predictor, weights=None, curvature=None, center=None, side=None, scale=None, window=None,
                 name="value"):
        self.cond_predictor = cond_predictor

        def arr(a, dtype=np.float32):
            return None if a is None else np.asarray(_to_numpy(a), dtype)

        self.weights, self.curvature, self.center = arr(weights), arr(curvature), arr(center)
        self.side = arr(side, np.int32)
        self.scale = None if scale is None else np.asarray(_to_numpy(scale), np.float32)
        self.window = None if window is None else (int(window[0]), int(window[1]))
        self.name = name

    @classmethod
    def from_physical(cls, cond_predictor, prop_dist: PropertyNorm, weights=None, curvature=None, center=None, side=None,
                      scale=None, window=None, name="value"):
        """The same target given in physical units of the properties: the predictor works on normalised properties
        p = (P - mean) / std (PropertyNorm), so  c -> (c - mean) / std,  q -> q std^2,  w -> w std  (the constant w . mean
        does not change the gradient and is dropped)."""
        mean, std = prop_dist.mean.astype(np.float32), prop_dist.std.astype(np.float32)
        conv = lambda a, f: None if a is None else f(np.asarray(_to_numpy(a), np.float32)).astype(np.float32)
        return cls(cond_predictor, conv(weights, lambda w: w * std), conv(curvature, lambda q: q * std * std),
                   conv(center, lambda c: (c - mean) / std), side, scale, window, name)

    def spec(self, scale=1.0) -> dict:
        """The engine's spec dict; ``scale`` (the sampling call's argument) multiplies the target's own."""
        sc = np.float32(scale) if self.scale is None else (self.scale * np.float32(scale)).astype(np.float32)
        return dict(w=self.weights, q=self.curvature, c=self.center, side=self.side, scale=sc, window=self.window)

    def value(self, pred: np.ndarray) -> np.ndarray:
        """T_b(pred_b) [B] in float32 (no scale: the reference's closures return the unscaled target)."""
        p = np.asarray(pred, np.float32)
        zero = np.zeros(p.shape[1], np.float32)
        w = zero if self.weights is None else self.weights
        q = zero if self.curvature is None else self.curvature
        c = zero if self.center is None else self.center
        sd = zero if self.side is None else self.side
        d = p - c
        a = np.where(sd == 0, d, np.where(sd > 0, np.where(d > 0, d, 0), np.where(d < 0, d, 0))).astype(np.float32)
        return ((w * p).sum(1, dtype=np.float32) + (q * a * a).sum(1, dtype=np.float32)).astype(np.float32)

    def grad(self, pred: np.ndarray, t: float = 0.0) -> np.ndarray:
        """dT/dpred [B,K] times the target's own scale, by the function the kernels use (engine.host_target_seed)."""
        from .engine import host_target_seed
        return host_target_seed(self.spec(), pred)

    def __call__(self, _input, _node_mask, _edge_mask, _t):
        pred = _to_numpy(self.cond_predictor(_input, _node_mask, _edge_mask, _t))
        return _like_ref(self.value(pred))


class ZTarget:
    """A target closure over (z, node_mask, edge_mask, t) that depends on z BOTH through the predictor and directly -- the
    reference differentiates any function of z_s (en_diffusion.py:899-903).  Per reverse step the host evaluates the closure on
    the device's z_s with the predictor output replaced by a leaf holding the device's prediction: torch.autograd then yields
    dT/dpred (fed to the GPU reverse pass) and the direct dT/dz (added to its result before the clip): gaudi_sample_cbz."""

    def __init__(self, cond_predictor, target, name="closure(z)"):
        self.cond_predictor = cond_predictor
        self.target = target
        self.name = name

    def grad(self, z, pred, t, node_mask, edge_mask):
        import torch
        cp = self.cond_predictor
        zt = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).requires_grad_(True)
        p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).requires_grad_(True)
        B = p.shape[0]
        cp._override, cp._override_used = p, False
        try:
            with torch.enable_grad():
                val = self.target(zt, torch.from_numpy(node_mask), torch.from_numpy(edge_mask), torch.full((B, 1), float(t)))
                gp, gz = torch.autograd.grad(val.sum(), (p, zt), allow_unused=True)
        finally:
            cp._override = None
        gp = np.zeros_like(pred) if gp is None else gp.detach().numpy().astype(np.float32)
        gz = np.zeros_like(z) if gz is None else gz.detach().numpy().astype(np.float32)
        return gp, gz

    def __call__(self, _input, _node_mask, _edge_mask, _t):
        return self.target(_input, _node_mask, _edge_mask, _t)


class PredTarget:
    """Arbitrary differentiable target T = fn(pred, t) of the predictor outputs (any closure the reference's
    sample_guidance accepts has this form, generation_guidance.py:187-211).  ``fn`` takes a torch tensor pred [B,K]
    (requires_grad) and the step time t and returns one value per molecule [B]; only its K-vector gradient is taken on
    the host (torch.autograd on a [B,K] leaf) -- the predictor forward and reverse passes stay on the GPU
    (gaudi_sample_cb)."""

    def __init__(self, cond_predictor, fn, name="custom"):
        self.cond_predictor = cond_predictor
        self.fn = fn
        self.name = name

    def grad(self, pred: np.ndarray, t: float) -> np.ndarray:
        import torch

        p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).requires_grad_(True)
        with torch.enable_grad():
            val = self.fn(p, t)
            (g,) = torch.autograd.grad(val.sum(), p, allow_unused=True)
        return np.zeros_like(pred) if g is None else g.detach().numpy().astype(np.float32)

    def __call__(self, _input, _node_mask, _edge_mask, _t):
        import torch

        pred = torch.from_numpy(_to_numpy(self.cond_predictor(_input, _node_mask, _edge_mask, _t)))
        t = float(np.asarray(_to_numpy(_t)).reshape(-1)[0]) if np.ndim(_to_numpy(_t)) else float(_t)
        return self.fn(pred, t)


class _DirectZ(Exception):
    pass


# autograd nodes a function that is affine in its leaf can be built from (name without the "BackwardN" suffix).  Anything else
# -- clamp, where, abs, threshold, relu, pow, exp ... -- is "not affine", whatever the numerical probes say: the backward pass of
# a mask-style kink (clamp / where / masked_fill) carries no grad_fn either, and random probes only see the side of the kink
# they land on.  Products / quotients of two pred-dependent factors pass this list and are caught by the
# differentiable-gradient check below.
_AFFINE_NODES = frozenset((
    "Neg", "Mul", "Add", "Sub", "Rsub", "Div", "Select", "Slice", "Index", "IndexSelect", "Gather", "Narrow", "Sum", "Mean",
    "View", "Reshape", "UnsafeView", "Squeeze", "Unsqueeze", "Expand", "Repeat", "T", "Transpose", "Permute", "Clone",
    "Contiguous", "Cat", "Stack", "Unbind", "Split", "SplitWithSizes", "Chunk", "ToCopy", "Alias", "Copy", "CopySlices",
    "AsStrided", "Mm", "Mv", "Dot", "Addmm", "Matmul", "Bmm", "Linear", "AccumulateGrad", "Flatten", "Unflatten", "Movedim",
    "Diagonal", "Flip", "Roll", "Addcmul"))


def _graph_is_affine(val) -> bool:
    """Every node of val's autograd graph is one a linear map is made of (no kinks, no transcendental functions)."""
    seen, todo = set(), [val.grad_fn]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        name = type(node).__name__
        cut = name.find("Backward")
        if (name[:cut] if cut >= 0 else name) not in _AFFINE_NODES:
            return False
        todo.extend(fn_ for fn_, _ in node.next_functions)
    return True


def _affine_probe(fn, p, t, ref):
    """One probe of affine_target_weights: -> dT/dpred of row 0 (== ref in every row when ref is given), or None."""
    import torch
    with torch.enable_grad():
        val = fn(p, t)
        if not torch.is_tensor(val) or not val.requires_grad or not _graph_is_affine(val):
            return None
        (g,) = torch.autograd.grad(val.sum(), p, create_graph=True, allow_unused=True)
    if g is None or g.requires_grad:
        return None  # no dependence on pred at all / the gradient depends on pred: not affine
    g = g.detach()
    if not bool(torch.isfinite(g).all()):
        return None
    if ref is None:
        ref = g[0].clone()
    return ref if bool((g == ref[None]).all()) else None


def affine_target_weights(fn, K: int, T: int, B: int = 3):
    """-> w [K] if fn(pred [B,K], t) -> [B] is  w . pred + c  with the same non-zero w for every molecule and every t, else
    None.  Three independent checks, all of which must hold: (i) the autograd graph of the value consists of linear nodes only
    (_AFFINE_NODES: a clamp / where / abs is refused by name, wherever its kink lies); (ii) dT/dpred does not depend on pred --
    asked for a differentiable gradient, it carries no grad_fn (all Hessian-vector products vanish identically); (iii)
    numerically: bit-equal gradients at random predictions of five very different magnitudes, at the first reverse step's
    t = 1, the last step's t = 1/T and one in between, and in every row of the batch.  w = 0 is 'not affine' too: the fused
    kernel would run an unguided chain where the callback path follows the closure faithfully (e.g. a closure that is
    switched off outside a window of t).  The probe visits three values of t; affine_gradient_holds() visits ALL of the
    chain's (GaudiModel._run runs it beside the device call).  Anything the probe cannot digest is 'not affine' (the general
    callback path, which is always correct)."""
    import torch
    gen = torch.Generator().manual_seed(1234)  # (torch's default generator keys the noise: not touched)
    ref = None
    try:
        for scale_p in (1.0, 1e-2, 30.0, 1e3, 1e6):
            for t in (1.0, 0.5, 1.0 / max(int(T), 1)):
                p = (torch.randn(B, K, generator=gen) * scale_p).requires_grad_(True)
                ref = _affine_probe(fn, p, t, ref)
                if ref is None:
                    return None
    except GaudiError:
        raise
    except Exception:
        return None
    if not bool((ref != 0).any()):
        return None
    return ref.numpy().astype(np.float32)


def affine_gradient_holds(fn, w, T: int, grid=None) -> bool:
    """The closure that affine_target_weights recognised, held to its weight vector at EVERY t the chain passes to it --
    (s + 1) / T as float32, s = 0 .. T-1 (gaudi_hip.hip: sample_cb_impl), or g[k] / T for every step of a time grid g (the
    last entry, 0, is where the chain lands: no step starts there) -- with rows of four magnitudes per call.  A closure
    whose python control flow depends on t (a guidance window) passes the three-point probe when the probe's points fall
    outside the window; this visits them all (T small torch evaluations; GaudiModel._run overlaps them with the device call)."""
    import torch
    K = int(len(w))
    ref = torch.from_numpy(np.asarray(w, np.float32))
    gen = torch.Generator().manual_seed(4321)
    base = torch.randn(4, K, generator=gen) * torch.tensor([[1.0], [1e-2], [30.0], [1e3]])
    try:
        t_indices = range(1, int(T) + 1) if grid is None else [int(g) for g in np.asarray(grid).reshape(-1)[:-1]]
        for t_idx in t_indices:
            t = float(np.float32(t_idx) / np.float32(T))
            if _affine_probe(fn, base.clone().requires_grad_(True), t, ref) is None:
                return False
    except GaudiError:
        raise
    except Exception:
        return False
    return True


def target_function_max_gap(cond_predictor) -> LinearTarget:
    """-pred[:,1]  (generation_guidance.py:200-203)."""
    w = np.zeros(cond_predictor.K, np.float32)
    w[1] = -1.0
    return LinearTarget(cond_predictor, w, name="max_gap")


def target_function_opv(cond_predictor, prop_dist: PropertyNorm) -> LinearTarget:
    """ip + ea + 3*gap on the un-normalised prediction (generation_guidance.py:205-211)."""
    w = np.zeros(cond_predictor.K, np.float32)
    w[0], w[2], w[3] = 3.0 * prop_dist.std[0], prop_dist.std[2], prop_dist.std[3]
    c = 3.0 * prop_dist.mean[0] + prop_dist.mean[2] + prop_dist.mean[3]
    return LinearTarget(cond_predictor, w, c, name="opv")


class GaudiModel:
    """Stands in for EnVariationalDiffusion on the sampling path: .sample / .sample_guidance / .normalize /
    .unnormalize / .T with the reference's signatures, and model(x, h, node_mask, edge_mask) -> the eval-mode NLL."""

    def __init__(self, args, state_dict, device: int = 0):
        self.args = checkpoint.args_dict(args)
        self.engine = Engine(device)
        self.engine.load_edm(self.args, state_dict)
        self.T = int(self.args["diffusion_steps"])
        self.in_node_nf = self.engine.F
        self.n_dims = 3
        self.norm_values = list(checkpoint.normalize_factors(self.args))
        self.norm_biases = (None, 0.0, 0.0)
        # Noise streams are keyed by (seed, global sample index, draw, element).  seed = None (default): every call draws its
        # 62-bit Philox key from torch's default generator, as the reference draws its noise from it (torch.randn,
        # en_diffusion.py:937-956): consecutive calls get fresh noise, torch.manual_seed(s) reproduces a run -- also when it
        # is called again with the SAME s between two calls (a stream position kept beside torch's seed
        # missed that) -- and anything else the caller draws from torch in between moves the key as it would move the
        # reference's noise.  An explicit seed (parity tests, sharded runs) keys the stream directly; then every call
        # consumes B fresh sample indices (sample_offset advances).
        self.seed = None
        self.sample_offset = 0
        self.injected_noise = None  # [T+2,B,N,3+F] raw draws (parity tests); None -> on-device Philox
        self.last_diag = None
        self.trace_guidance = False  # True: a ValueTarget chain also records its guidance trace ...
        self.last_trace = None       # ... here: [steps, B, K+2] (Engine.sample_target)
        self._state = state_dict
        import weakref
        GaudiModel._latest = weakref.ref(self)

    _latest = None

    @classmethod
    def from_engine(cls, engine: Engine, args) -> "GaudiModel":
        """A model object over an Engine whose EDM weights are already loaded (bench.py: one handle serves several drivers)."""
        m = cls.__new__(cls)
        m.args = checkpoint.args_dict(args)
        m.engine = engine
        m.T = int(m.args["diffusion_steps"])
        m.in_node_nf = engine.F
        m.n_dims = 3
        m.norm_values = list(checkpoint.normalize_factors(m.args))
        m.norm_biases = (None, 0.0, 0.0)
        m.seed, m.sample_offset, m.injected_noise, m.last_diag = None, 0, None, None
        m.trace_guidance, m.last_trace = False, None
        return m

    @classmethod
    def latest(cls):
        """The GaudiModel created last that is still alive (what get_cond_predictor_model(args, dataset) attaches to)."""
        m = cls._latest() if cls._latest is not None else None
        return m if m is not None and getattr(m.engine, "h", None) else None

    def _trace_closure(self, target):
        """An opaque target closure over (z, node_mask, edge_mask, t), as generation_guidance.py:198-211 writes them
        (``lambda z, nm, em, t: -cond_predictor(z, nm, em, t)[:, 1]``), turned into a PredTarget: while the closure runs, the
        predictor attached to this model returns a stand-in tensor, so torch.autograd yields dT/dpred for the GPU reverse
        pass.  The closure may be ANY differentiable torch function of the predictor outputs and t: affine ones run fused
        (LinearTarget), the others through the per-step callback (PredTarget); one that ALSO depends on z outside the
        predictor becomes a ZTarget (the host adds its direct dT/dz, gaudi_sample_cbz)."""
        cp = getattr(self, "cond_predictor", None)
        if cp is None:
            raise GaudiError("guidance with a target closure needs get_cond_predictor_model(...) on this model first")
        model = self

        def fn(pred, t):
            import torch
            B = pred.shape[0]
            # stand-in z (deterministic, non-zero: a direct dependence must show up in its gradient; torch's default generator
            # is not touched -- it keys the noise).  The stand-ins depend on (B, masks) only: built once per call, not per step.
            cache, key = model.__dict__.setdefault("_trace_cache", {}), B  # (_run empties it whenever it sets new masks)
            if cache.get("key") != key:
                shape = (B, model._trace_N, 3 + model.in_node_nf)
                nm_all, em_all = model._trace_nm, model._trace_em.reshape(model._trace_nm.shape[0], -1, 1)
                rows = np.arange(B) % nm_all.shape[0]  # (the affine probe runs on a few rows only)
                cache.update(key=key,
                             probe=(0.25 + torch.linspace(0.0, 1.0, int(np.prod(shape))).reshape(shape)).requires_grad_(True),
                             nm=torch.from_numpy(np.ascontiguousarray(nm_all[rows])),
                             em=torch.from_numpy(np.ascontiguousarray(em_all[rows]).reshape(-1, 1)))
            probe, nm, em = cache["probe"], cache["nm"], cache["em"]
            cp._override, cp._override_used = pred, False
            try:
                val = target(probe, nm, em, torch.full((B, 1), float(t)))
            finally:
                cp._override = None
            if not torch.is_tensor(val) or val.dim() == 0 or val.shape[0] != B:
                raise GaudiError("the target function must return one value per molecule (a torch tensor [B]); use a "
                                 "LinearTarget / PredTarget or a closure over cond_predictor (generation_guidance.py:198-211)")
            if val.requires_grad:
                (gz,) = torch.autograd.grad(val.sum(), probe, allow_unused=True, retain_graph=True)
                if gz is not None and bool((gz != 0).any()):
                    raise _DirectZ()  # depends on z outside cond_predictor too: the general form (ZTarget)
            # The closure must route through the predictor attached to THIS model: one that closes over another predictor (or a
            # torch module, or uses t only) would give dT/dpred = 0 here and the chain would run unguided without a word.
            if not cp._override_used or (pred.requires_grad and not val.requires_grad):
                raise GaudiError("the target function does not use the predictor attached to this model (it must call the "
                                 "cond_predictor returned by get_cond_predictor_model(..., model=<this model>)): its value does "
                                 "not depend on the prediction, guidance would be a no-op")
            return val

        pt = PredTarget(cp, fn, name=getattr(target, "__name__", "closure"))
        try:  # one probe evaluation: does the closure route through the predictor, does it depend on z directly?
            import torch
            fn(torch.zeros(min(2, int(self._trace_nm.shape[0])), cp.K).requires_grad_(True), 0.5)
        except _DirectZ:
            return ZTarget(cp, target, name=pt.name + " (direct z dependence)")
        lin = affine_target_weights(pt.fn, cp.K, self.T)
        if lin is not None:
            # affine in pred and independent of t (both closures the reference ships are, generation_guidance.py:200-211): the
            # declarative form, whose guidance is fused into the step kernel (one launch per 25 steps, no host round trip)
            lt = LinearTarget(cp, lin, name=pt.name + " (affine: fused)")
            lt._closure_fn = pt.fn  # _run re-checks the closure's gradient at the predictions the chain ends on
            return lt
        return pt

    # ---- training (train_edm.py:52-94).  Unlike an nn.Module, a GaudiModel starts in eval mode: model(...) is the eval-mode
    # NLL until train() is called.  The parameters are torch tensors on the host in the reference's names (gamma.gamma with
    # requires_grad=False, then every dynamics.egnn tensor); changes made in place (optimizer.step(), load_state_dict) reach
    # the training kernels through Engine.edm_set_train_weights before the next EDM call, and the sampler's images are
    # rebuilt (Engine.load_edm) only before the next sampler-kernel call.
    training = False
    _state = None   # the state dict the model was built from (None: from_engine, nothing to train)
    _params = None  # name -> torch.nn.Parameter, created on first use
    _pushed = None  # the parameters' version counters when the device copy was last set

    def _ensure_params(self):
        if self._params is None:
            if self._state is None:
                raise GaudiError("training needs the host copy of the weights: a model built with from_engine has none")
            import collections
            import torch
            from .engine import _strip
            sd = _strip(self._state)
            gamma = sd.get("gamma.gamma")
            if gamma is None:
                gamma = self.engine.gamma().astype(np.float32)
            params = collections.OrderedDict()
            params["gamma.gamma"] = torch.nn.Parameter(torch.from_numpy(np.array(gamma, np.float32)), requires_grad=False)
            for k in self.engine.edm_names:
                if k.startswith("dynamics."):
                    params[k] = torch.nn.Parameter(torch.from_numpy(sd[k].copy()))
            self._buffer = torch.from_numpy(np.asarray(sd.get("buffer", np.zeros(1, np.float32)), np.float32).copy())
            self._params = params
            self._pushed = self._versions()
            self.engine.edm_sync = self._sync
        return self._params

    def _versions(self):
        return tuple(p._version for p in self._params.values())

    def _sync(self):
        """Parameters changed in place reach the training kernels (no repack) before the next EDM call."""
        if self._params is not None and self._versions() != self._pushed:
            self._pushed = self._versions()
            sd = {}
            for k in self.engine.edm_names:
                if k in self._params:
                    sd[k] = self._params[k].detach().numpy()
                elif k == "buffer":
                    sd[k] = self._buffer.numpy()
            self.engine.edm_set_train_weights(sd)

    def named_parameters(self):
        """(name, torch.nn.Parameter) in the reference's names and order (EnVariationalDiffusion.named_parameters)."""
        return iter(self._ensure_params().items())

    def parameters(self):
        return iter(self._ensure_params().values())

    def state_dict(self):
        """A copy in the reference's keys (buffer, gamma.gamma, dynamics.*) that its strict load_state_dict and get_model
        accept."""
        import collections
        params = self._ensure_params()
        out = collections.OrderedDict(buffer=self._buffer.clone())
        for k, p in params.items():
            out[k] = p.detach().clone()
        return out

    def load_state_dict(self, state_dict, strict: bool = True):
        import torch
        from .engine import _strip
        params = self._ensure_params()
        sd = _strip(state_dict)
        missing = set(params) - set(sd)
        if missing or (strict and set(sd) - set(params) - {"buffer"}):
            raise GaudiError(f"load_state_dict: keys differ from the model's: {sorted(set(sd) ^ set(params))[:4]}")
        with torch.no_grad():
            for k, p in params.items():
                p.copy_(torch.from_numpy(sd[k]))
        self._sync()

    def train(self, mode: bool = True):
        """model(...) then returns the train-mode loss per molecule (compute_loss with t0_always=False), whose backward()
        fills every dynamics.* .grad; train(False) = eval()."""
        if mode:
            loss_type = self.args.get("diffusion_loss_type", "l2")
            if loss_type not in ("l2", "vlb"):
                raise GaudiError(f"diffusion_loss_type must be 'l2' or 'vlb', got {loss_type!r}")
            self._ensure_params()
        self.training = bool(mode)
        return self

    def eval(self):
        """Back to the eval-mode NLL (two network passes, no reverse pass)."""
        return self.train(False)

    def _train_forward(self, xn, hc, nm, em):
        """en_diffusion.py:777-792 in train mode -> the per-molecule loss [B] through _EdmLoss."""
        import torch
        B = xn.shape[0]
        params = self._ensure_params()
        loss_type = self.args.get("diffusion_loss_type", "l2")
        t_int = torch.randint(0, self.T + 1, size=(B, 1)).float()  # t0_always=False: t = 0 included (:657-659)
        ti = t_int.numpy().reshape(B).astype(np.int32)
        noise = self.injected_noise
        noise = None if noise is None or np.shape(noise)[0] != 1 else np.asarray(noise)[0]  # [1,B,N,3+F]: ONE draw
        seed, off = self.next_stream(B)

        def call(weight=None):
            return self.engine.edm_loss_grad(xn, hc, ti, nm, em, seed=seed, sample_offset=off, noise=noise,
                                             loss_type=loss_type, weight=weight)

        loss, _, grads = call()
        names = list(params)
        g = tuple(None if grads.get(k) is None else torch.from_numpy(grads[k]) for k in names)
        return _edm_loss_apply(torch.from_numpy(loss), (names, g, call), *params.values())

    # ---- en_diffusion.py:777-805 (eval mode)
    def forward(self, x, h, node_mask=None, edge_mask=None, context=None):
        """EnVariationalDiffusion.forward in eval mode -> the negative log-likelihood per molecule, a torch tensor [B].
        t_int ~ U{1..T} is drawn with torch.randint as the reference draws it (torch.manual_seed reproduces its t); the two noise
        draws come from this model's stream (next_stream), or from injected_noise when that holds [2,B,N,3+F] raw draws."""
        import torch
        if context is not None:
            raise GaudiError("context conditioning is not part of this port")
        if not isinstance(h, dict) or "categorical" not in h:
            raise GaudiError('h must be the reference\'s dict {"categorical": [B,N,F], "integer": ...}')
        hi = h.get("integer")
        if hi is not None and np.size(_to_numpy(hi)) != 0:
            raise GaudiError("include_charges is False for GaUDI checkpoints (models_edm.py:94): h['integer'] must be empty")
        xn = _to_numpy(x).astype(np.float32)
        B, N = xn.shape[0], xn.shape[1]
        if node_mask is None or edge_mask is None:
            raise GaudiError("node_mask and edge_mask are required")
        nm = _to_numpy(node_mask).astype(np.float32).reshape(B, N)
        em = _to_numpy(edge_mask).astype(np.float32).reshape(B, N, N)
        hc = _to_numpy(h["categorical"]).astype(np.float32).reshape(B, N, self.in_node_nf)
        assert_correctly_masked(hc, nm)
        assert_mean_zero_with_mask(xn, nm)  # (compute_loss asserts it on z_t, en_diffusion.py:680)
        if self.training:
            return self._train_forward(xn, hc, nm, em)
        t_int = torch.randint(1, self.T + 1, size=(B, 1)).float()  # t0_always: lowest_t = 1 (:651-659)
        noise = self.injected_noise
        if noise is None or np.shape(noise)[0] != 2:
            noise = None
        seed, off = self.next_stream(B)
        nll = self.engine.edm_nll(xn, hc, t_int.numpy().reshape(B).astype(np.int32), nm, em, seed=seed, sample_offset=off,
                                  noise=noise)
        return _like_ref(nll)

    __call__ = forward

    # ---- en_diffusion.py:384-415
    def normalize(self, x, h, node_mask):
        x = _to_numpy(x) / self.norm_values[0]
        nm = _to_numpy(node_mask)
        h_cat = (_to_numpy(h["categorical"]).astype(np.float32) - self.norm_biases[1]) / self.norm_values[1] * nm
        return _like_ref(x.astype(np.float32)), {"categorical": _like_ref(h_cat.astype(np.float32)),
                                                  "integer": h.get("integer")}, None

    def unnormalize(self, x, h_cat, h_int, node_mask):
        nm = _to_numpy(node_mask)
        x = _to_numpy(x) * self.norm_values[0]
        h_cat = (_to_numpy(h_cat) * self.norm_values[1] + self.norm_biases[1]) * nm
        return _like_ref(x), _like_ref(h_cat), h_int

    def next_stream(self, n_samples: int):
        """-> (seed, sample_offset) for a call that draws noise for ``n_samples`` molecules; advances the offset."""
        if self.seed is None:
            import torch
            return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()), 0
        off = self.sample_offset
        self.sample_offset += int(n_samples)
        return int(self.seed), off

    def _run(self, n_samples, node_mask, edge_mask, std, target, scale, fix_noise, grid=None, start=None):
        """grid: the time grid the chain runs on (None: all T steps, today's entry points); start = (x, onehot): given
        molecules the chain starts from, noised to grid[0], instead of the prior."""
        gk = {} if grid is None else dict(grid=np.ascontiguousarray(np.asarray(grid).reshape(-1), dtype=np.int32), start=start)
        nm = _to_numpy(node_mask).astype(np.float32)
        B, N = nm.shape[0], nm.shape[1]
        if B != n_samples:
            raise GaudiError(f"n_samples={n_samples} but node_mask has batch {B}")
        em = _to_numpy(edge_mask).astype(np.float32).reshape(B, N, N)
        tw = None
        if target is not None:
            if not isinstance(target, (LinearTarget, PredTarget, ZTarget, ValueTarget)):
                if not callable(target):
                    raise GaudiError("target_function must be callable")
                # the reference's own form: a closure over (z, node_mask, edge_mask, t) that calls cond_predictor
                self._trace_N, self._trace_nm, self._trace_em = N, nm.reshape(B, N, 1), em.reshape(B * N * N, 1)
                self._trace_cache = {}
                target = self._trace_closure(target)
            if target.cond_predictor.engine is not self.engine:
                raise GaudiError("the target's predictor must be attached to this model (get_cond_predictor_model(..., model=model))")
        seed, off = self.next_stream(B)
        # fix_noise (en_diffusion.py:562-566,972-978): one raw draw per call, broadcast over the batch
        self.engine.set_fix_noise(bool(fix_noise), off)
        try:
            self.last_trace = None
            if isinstance(target, ValueTarget):
                out = self.engine.sample_target(nm.reshape(B, N), em, target.spec(scale), seed=seed, sample_offset=off,
                                                noise=self.injected_noise, std=std, trace=bool(self.trace_guidance), **gk)
                x, h, diag = out[0], out[1], out[2]
                if self.trace_guidance:
                    self.last_trace = out[-1]  # [steps, B, K+2]: predictions | gradient norm before the clip | clip coefficient
            elif isinstance(target, ZTarget):
                nm3, em_flat = nm.reshape(B, N, 1), em.reshape(B * N * N, 1)
                x, h, diag = self.engine.sample_callback(nm.reshape(B, N), em, lambda z, p, t: target.grad(z, p, t, nm3, em_flat),
                                                         seed=seed, sample_offset=off, noise=self.injected_noise, std=std,
                                                         scale=scale, with_z=True, **gk)
            elif isinstance(target, PredTarget):
                x, h, diag = self.engine.sample_callback(nm.reshape(B, N), em, target.grad, seed=seed, sample_offset=off,
                                                         noise=self.injected_noise, std=std, scale=scale, **gk)
            else:
                tw = None if target is None else target.weights
                fn = getattr(target, "_closure_fn", None)
                holds, checker = [True], None
                if fn is not None:
                    # the closure was recognised as affine at three values of t; while the device runs the fused chain, the host
                    # holds it to that weight vector at every t of the chain (a closure with a guidance window).
                    # NOTE for callers: the closure is evaluated on a helper thread beside the engine call (it only ever sees
                    # stand-in predictions, never the engine) -- a closure with side effects on shared state must be wrapped in
                    # PredTarget.  The verdict is cached per (closure, T, weights, time grid): repeated calls of design() with the
                    # same closure pay for it once; another grid visits other t and is checked on its own.
                    import threading
                    key = (id(fn), int(self.T), tw.tobytes(), None if grid is None else gk["grid"].tobytes())
                    cache = self.__dict__.setdefault("_affine_verdicts", {})
                    if key in cache and cache[key][0] is fn:
                        holds[0] = cache[key][1]
                    else:
                        def _check_all_t():
                            try:
                                holds[0] = affine_gradient_holds(fn, tw, self.T, gk.get("grid"))
                            except BaseException:
                                holds[0] = False
                        checker = threading.Thread(target=_check_all_t, daemon=True)
                        checker.start()
                try:
                    out = self.engine.sample(nm.reshape(B, N), em, seed=seed, sample_offset=off, noise=self.injected_noise, std=std,
                                             target_w=tw, scale=scale, return_z0=fn is not None, **gk)
                finally:
                    if checker is not None:  # (joined whether or not the engine call raised)
                        checker.join()
                        if len(cache) > 64:
                            cache.clear()
                        cache[key] = (fn, holds[0])  # (the closure object is kept: its id cannot be reused while cached)
                x, h, diag = out[0], out[1], out[2]
                if fn is not None and not holds[0]:
                    # not the affine function the probe saw: the fused result is discarded and the SAME call (same noise stream)
                    # runs through the general path, which differentiates the closure at every step
                    pt = PredTarget(target.cond_predictor, fn, name=target.name + " -> callback")
                    x, h, diag = self.engine.sample_callback(nm.reshape(B, N), em, pt.grad, seed=seed, sample_offset=off,
                                                             noise=self.injected_noise, std=std, scale=scale, **gk)
                    diag = dict(diag, affine_recheck_failed=1)
                elif fn is not None:
                    # ... and at the predictions the chain actually ended on
                    import torch
                    # (the t of the last step: 1 / T on the unit grid, g[n-1] / T on a time grid)
                    t_last = 1.0 / self.T if grid is None else float(np.float32(gk["grid"][-2]) / np.float32(self.T))
                    p0 = torch.from_numpy(self.engine.predictor_fwd(out[3], t_last, nm.reshape(B, N), em)).requires_grad_(True)
                    with torch.enable_grad():
                        (g0,) = torch.autograd.grad(fn(p0, t_last).sum(), p0, allow_unused=True)
                    if g0 is None or not bool((g0 == torch.from_numpy(tw)[None]).all()):
                        raise GaudiError("the target closure was run as an affine function of the predictor outputs, but its "
                                         "gradient at the final predictions differs from the probed one: wrap it in "
                                         "PredTarget(cond_predictor, fn) to force the general path")
        finally:
            self.engine.set_fix_noise(False, 0)
        self.last_diag = diag
        F = h.shape[2]
        return _like_ref(x), {"categorical": _like_ref(h), "integer": _like_ref(np.zeros((B, N, 0), np.float32))}

    def sample(self, n_samples, n_nodes, node_mask, edge_mask, context=None, fix_noise=False, std=1.0, grid=None):
        """EnVariationalDiffusion.sample (en_diffusion.py:958-1008); grid: a time grid (sampling_edm.time_grid) to run the
        chain on instead of all T steps."""
        if context is not None:
            raise GaudiError("context conditioning is not part of the GaUDI sampling path")
        return self._run(n_samples, node_mask, edge_mask, std, None, 1.0, fix_noise, grid=grid)

    def sample_chain(self, n_samples, n_nodes, node_mask, edge_mask, context, keep_frames=None, std=1.0):
        """EnVariationalDiffusion.sample_chain (en_diffusion.py:1118-1174) -> chain_flat [keep_frames*n_samples, N, 3+F]."""
        if context is not None:
            raise GaudiError("context conditioning is not part of the GaUDI sampling path")
        nm = _to_numpy(node_mask).astype(np.float32)
        B, N = nm.shape[0], nm.shape[1]
        K = self.T if keep_frames is None else int(keep_frames)
        assert K <= self.T
        seed, off = self.next_stream(B)
        chain = self.engine.sample_chain(nm.reshape(B, N), _to_numpy(edge_mask).astype(np.float32).reshape(B, N, N), K,
                                         seed=seed, sample_offset=off, noise=self.injected_noise, std=std)
        return _like_ref(chain.reshape(K * B, N, chain.shape[-1]))

    def sample_guidance(self, n_samples, target_function, node_mask, edge_mask, scale=1, fix_noise=False, std=1.0, grid=None):
        """EnVariationalDiffusion.sample_guidance (en_diffusion.py:1010-1067); grid as in sample()."""
        return self._run(n_samples, node_mask, edge_mask, std, target_function, scale, fix_noise, grid=grid)

    def refine(self, x, h, node_mask, edge_mask, t_start, target_function=None, scale=1, n_steps=None):
        """Start from given molecules instead of the prior: remove the masked mean of x, noise (x, h) to time index t_start
        as sample_edm_t does (cond_prediction/train_cond_predictor.py:47-61; it has no std), then run the reverse process
        -- guided when target_function is given -- from there down to 0 in n_steps steps (default: all t_start).  Costs
        t_start / T of a full chain.  h: the one-hot features [B,N,F] or the reference's dict.  Returns what sample_guidance
        returns."""
        from .sampling_edm import time_grid
        xn = _to_numpy(x).astype(np.float32)
        B, N = xn.shape[0], xn.shape[1]
        nm = _to_numpy(node_mask).astype(np.float32).reshape(B, N)
        hc = _to_numpy(h["categorical"] if isinstance(h, dict) else h).astype(np.float32).reshape(B, N, self.in_node_nf)
        # as the reference's training loops prepare a batch (train_cond_predictor.py:64-71): centre, then check the masking
        xn = xn * nm[:, :, None]
        xn = xn - (xn.sum(1, keepdims=True) / np.maximum(nm.sum(1), 1.0)[:, None, None]) * nm[:, :, None]
        assert_correctly_masked(hc, nm)
        assert_mean_zero_with_mask(xn, nm)
        t_start = int(t_start)
        grid = time_grid(self.T, t_start if n_steps is None else int(n_steps), t_start)
        return self._run(B, nm.reshape(B, N, 1), edge_mask, 1.0, target_function, scale, False, grid=grid, start=(xn, hc))


def assert_correctly_masked(variable, node_mask):
    """utils.py:63-66 as a GaudiError: no value outside the mask."""
    v = _to_numpy(variable).astype(np.float32)
    nm = _to_numpy(node_mask).astype(np.float32).reshape(v.shape[0], v.shape[1], 1)
    if v.size and float(np.abs(v * (1 - nm)).max()) >= 1e-4:
        raise GaudiError("Variables not masked properly.")


def assert_mean_zero_with_mask(x, node_mask, eps=1e-10):
    """utils.py:52-60 as a GaudiError: the masked positions have zero centre of gravity."""
    assert_correctly_masked(x, node_mask)
    x = _to_numpy(x).astype(np.float32)
    largest = float(np.abs(x).max()) if x.size else 0.0
    err = float(np.abs(x.sum(1, keepdims=True)).max()) if x.size else 0.0
    rel = err / (largest + eps)
    if not rel < 1e-2:
        raise GaudiError(f"Mean is not zero, relative_error {rel}")


class CondPredictor:
    """Stands in for EGNN_predictor: callable (xh, node_mask, edge_mask, t) -> pred [B,K] (models.py:433-457)."""

    def __init__(self, model: GaudiModel, args, state_dict):
        self.args = checkpoint.args_dict(args)
        self.engine = model.engine
        self.engine.load_predictor(self.args, state_dict)
        self.K = self.engine.K
        self._state = state_dict

    training = False
    _params = None  # name -> torch.nn.Parameter, created on first use (parameters(), state_dict(), train())
    _pushed = None  # the parameters' version counters when the device copy was last loaded

    def _ensure_params(self):
        if self._params is None:
            if self._state is None:
                raise GaudiError("a predictor attached with from_engine has no host copy of its weights to train")
            import torch
            from .engine import _strip
            sd = _strip(self._state)
            self._params = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in sd.items()}
            self._pushed = self._versions()
            self.engine.pred_sync = self._sync
        return self._params

    def _versions(self):
        return tuple(p._version for p in self._params.values())

    def _sync(self):
        """Parameters changed in place (optimizer.step(), load_state_dict) reach the device before the next predictor call."""
        if self._params is not None and self._versions() != self._pushed:
            sd = {k: p.detach().numpy() for k, p in self._params.items()}
            self._pushed = self._versions()
            self.engine.load_predictor(self.args, sd)

    def named_parameters(self):
        """(name, torch.nn.Parameter) in the reference's state-dict names (EGNN_predictor.named_parameters)."""
        return iter(self._ensure_params().items())

    def parameters(self):
        return iter(self._ensure_params().values())

    def state_dict(self):
        """A copy that get_cond_predictor_model (and the reference's EGNN_predictor.load_state_dict) reloads."""
        import collections
        return collections.OrderedDict((k, p.detach().clone()) for k, p in self._ensure_params().items())

    def load_state_dict(self, state_dict):
        import torch
        from .engine import _strip
        params = self._ensure_params()
        sd = _strip(state_dict)
        if set(sd) != set(params):
            raise GaudiError(f"load_state_dict: names differ from the predictor's: {sorted(set(sd) ^ set(params))[:4]}")
        with torch.no_grad():
            for k, p in params.items():
                p.copy_(torch.from_numpy(sd[k]))
        self._sync()

    def train(self, mode: bool = True):
        """compute_loss then returns a loss whose backward() fills p.grad (gaudi_amd/cond_prediction.py); train(False) = eval()."""
        if mode:
            self._ensure_params()
        self.training = bool(mode)
        return self

    @classmethod
    def from_engine(cls, model: GaudiModel, args) -> "CondPredictor":
        """Over a model whose engine already holds the predictor weights; attaches itself to the model."""
        cp = cls.__new__(cls)
        cp.args = checkpoint.args_dict(args)
        cp.engine = model.engine
        cp.K = model.engine.K
        cp._state = None
        model.cond_predictor = cp
        return cp

    def eval(self):
        """Back to the forward-only path: compute_loss / val_epoch evaluate without the reverse pass."""
        return self.train(False)

    _override = None  # set while a target closure is being traced (GaudiModel._trace_closure): the stand-in prediction

    def __call__(self, xh, node_mask, edge_mask, t=0.0):
        if self._override is not None:
            self._override_used = True
            return self._override
        z = _to_numpy(xh).astype(np.float32)
        B, N, _ = z.shape
        tt = np.broadcast_to(_to_numpy(t).astype(np.float32).reshape(-1), (B,)) if np.ndim(_to_numpy(t)) else float(t)
        return _like_ref(self.engine.predictor_fwd(z, tt, _to_numpy(node_mask).reshape(B, N),
                                                   _to_numpy(edge_mask).reshape(B, N, N)))


_EDM_LOSS = None  # the torch.autograd.Function below, built on first use (torch is imported lazily here)


def _edm_loss_apply(loss, ctx_data, *params):
    global _EDM_LOSS
    if _EDM_LOSS is None:
        _EDM_LOSS = _make_edm_loss()
    return _EDM_LOSS.apply(loss, ctx_data, *params)


def _make_edm_loss():
    import torch

    class _EdmLoss(torch.autograd.Function):
        """The per-molecule loss of gaudi_edm_loss_grad as a function of the parameters.  The forward call kept
        G = sum_b g_b; an incoming gradient c that is the same for every molecule (loss.mean(0), loss.sum()) gives c G, any
        other one re-runs the call with weight = grad_output (same t, noise stream or injected noise)."""

        @staticmethod
        def forward(ctx, loss, data, *ps):
            ctx.data = data
            return loss.clone()

        @staticmethod
        def backward(ctx, go):
            names, grads, call = ctx.data
            if bool(torch.all(go == go.reshape(-1)[0])):
                c = go.reshape(-1)[0]
                out = tuple(None if g is None else g * c for g in grads)
            else:
                rerun = call(weight=go.detach().numpy().astype(np.float32).reshape(-1))[2]
                out = tuple(None if rerun.get(k) is None else torch.from_numpy(rerun[k]) for k in names)
            return (None, None) + out

    return _EdmLoss


def init_edm_state_dict(args, in_node_nf: int) -> dict:
    """Fresh weights of EGNN_dynamics drawn as the reference's modules draw them from torch's default generator, in
    construction order (egnn_new.py:268-312 EGNN, 194-222 EquivariantBlock, 6-44 GCL, 96-121 EquivariantUpdate: its
    bias-free last layer, xavier with gain 0.001, is built BEFORE coord_mlp's first two linears).  nn.Linear itself draws
    them, so the numbers are torch's; gamma.gamma is the schedule table and buffer zero (en_diffusion.py:216-218)."""
    import torch
    a = checkpoint.args_dict(args)
    H, L, S = int(a["nf"]), int(a["n_layers"]), int(a.get("inv_sublayers", 1))
    A = 24 if a.get("sin_embedding") else 2
    F1 = int(in_node_nf) + 1
    sd = {"buffer": np.zeros(1, np.float32)}

    def lin(name, i, o, layer=None):
        m = layer if layer is not None else torch.nn.Linear(i, o)
        sd[name + ".weight"] = m.weight.detach().numpy().copy()
        if m.bias is not None:
            sd[name + ".bias"] = m.bias.detach().numpy().copy()

    p = "dynamics.egnn."
    lin(p + "embedding", F1, H)
    lin(p + "embedding_out", H, F1)
    for l in range(L):
        b = f"{p}e_block_{l}."
        for s in range(S):
            q = f"{b}gcl_{s}."
            lin(q + "edge_mlp.0", 2 * H + A, H)
            lin(q + "edge_mlp.2", H, H)
            lin(q + "node_mlp.0", 2 * H, H)
            lin(q + "node_mlp.2", H, H)
            if a["attention"]:
                lin(q + "att_mlp.0", H, 1)
        last = torch.nn.Linear(H, 1, bias=False)
        torch.nn.init.xavier_uniform_(last.weight, gain=0.001)
        q = f"{b}gcl_equiv.coord_mlp."
        lin(q + "0", 2 * H + A, H)
        lin(q + "2", H, H)
        lin(q + "4", H, 1, layer=last)
    return sd


def get_model(args, dataloader_train=None, only_norm=True, device: int = 0, state_dict=None):
    """models_edm.get_model (models_edm.py:61-104) -> (model, nodes_dist, prop_dist).

    ``dataloader_train.dataset`` is only consulted for ``mean``/``std`` (property normalisation) and, without a checkpoint,
    for ``num_node_features``.  Without args.restore or a state dict the model starts from fresh weights
    (init_edm_state_dict), as the reference's does."""
    a = checkpoint.args_dict(args)
    if state_dict is None:
        if a.get("restore"):
            state_dict = checkpoint.load_state_dict(a["exp_dir"])
        else:
            ds = getattr(dataloader_train, "dataset", None)
            F = getattr(ds, "num_node_features", None)
            if F is None:
                from . import synth
                F = synth.num_node_features(a.get("dataset", "cata"))
            state_dict = init_edm_state_dict(a, int(F))
    model = GaudiModel(a, state_dict, device=device)
    prop_dist = None
    ds = getattr(dataloader_train, "dataset", None)
    if ds is not None and getattr(ds, "mean", None) is not None:
        prop_dist = PropertyNorm(ds.mean, ds.std)
    return model, DistributionRings(a.get("dataset", "cata")), prop_dist


def get_cond_predictor_model(args, dataset=None, model: GaudiModel | None = None, state_dict=None) -> CondPredictor:
    """cond_prediction/train_cond_predictor.py:183-203 with the reference's own call shape ``(args, dataset)``: the predictor
    is attached to a GaudiModel's GPU handle so that guidance runs inside the same kernel launch as the denoiser --
    ``model`` if given, otherwise the model ``get_model`` created last (the order of generation_guidance.py:190-195)."""
    if model is None:
        model = GaudiModel.latest()
        if model is None:
            raise GaudiError("get_cond_predictor_model: call get_model first (the predictor shares the EDM's device handle) "
                             "or pass model=<GaudiModel>")
    a = checkpoint.args_dict(args)
    if state_dict is None:
        state_dict = checkpoint.load_state_dict(a["exp_dir"])
    model.cond_predictor = CondPredictor(model, a, state_dict)
    return model.cond_predictor
