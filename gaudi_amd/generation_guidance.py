"""Host mirror of generation_guidance.py: predict / get_target_function_values / design.  The reference filters the
designed molecules with RDKit validity (eval_stability, generation_guidance.py:69-80); RDKit is not a dependency here, so
the filter is the graph-of-rings stability check of eval_validity.py on the GPU (gaudi_amd.analyze), and plots are replaced
by the returned dict.  With ``with_atoms=True`` the designed molecules also come back as graphs of atoms (gaudi_amd.gor2goa,
hydrogens placed) with fingerprints and ``mol_unique``, and with ``valence_check=True`` on top of it with the valence check the
reference makes through xyz2mol (bond orders and formal charges per molecule, ``mol_valid``, ``valid``, ``best_valid``); RDKit
itself (its sanitiser, InChI) is still missing."""
from __future__ import annotations

from time import time

import numpy as np

from .analyze import analyze_validity_for_molecules
from .models_edm import _like_ref, _to_numpy
from .sampling_edm import _check, sample_guidance


def _normalized_xh(x, h, node_mask, edm_model):
    x, hh, _ = edm_model.normalize(x, {"categorical": h, "integer": None}, node_mask)
    return np.concatenate([_to_numpy(x), _to_numpy(hh["categorical"])], axis=-1).astype(np.float32)


def predict(model, x, h, node_mask, edge_mask, edm_model):
    """generation_guidance.py:34-48: predictor at t=0 on the normalised sample."""
    bs, n_nodes, _ = _to_numpy(x).shape
    nm = _to_numpy(node_mask).reshape(bs, n_nodes, 1)
    em = _to_numpy(edge_mask).reshape(bs, n_nodes * n_nodes)
    return model(_normalized_xh(x, h, nm, edm_model), nm, em, np.zeros((bs, 1), np.float32))


def get_target_function_values(x, h, target_function, node_mask, edge_mask, edm_model):
    """generation_guidance.py:51-66."""
    bs, n_nodes, _ = _to_numpy(x).shape
    nm = _to_numpy(node_mask).reshape(bs, n_nodes, 1)
    em = _to_numpy(edge_mask).reshape(bs, n_nodes * n_nodes)
    # torch tensors, as the reference passes them: a target closure may combine them with the (torch) prediction
    return target_function(_like_ref(_normalized_xh(x, h, nm, edm_model)), _like_ref(nm.astype(np.float32)),
                           _like_ref(em.astype(np.float32)), _like_ref(np.zeros((bs, 1), np.float32)))


def eval_stability(x, one_hot, node_mask, edge_mask, dataset="cata", engine=None):
    """generation_guidance.py:69-80 with the graph-of-rings check in place of RDKit validity:
    -> (stability_dict, x, one_hot, node_mask, edge_mask) of the stable molecules."""
    import torch
    bs, n, _ = x.shape
    atom_type = one_hot.argmax(2)
    keep = [node_mask[i, :, 0].bool() for i in range(bs)]
    molecule_list = [(x[i][keep[i]], atom_type[i][keep[i]]) for i in range(bs)]
    stability_dict, _ = analyze_validity_for_molecules(molecule_list, dataset=dataset, engine=engine)
    ok = torch.tensor(stability_dict["molecule_stable_bool"], dtype=torch.bool)
    return stability_dict, x[ok], one_hot[ok], node_mask[ok], edge_mask.view(bs, n, n)[ok].view(-1, 1)


def design(args, model, cond_predictor, target_function, nodes_dist, prop_dist, scale, n_nodes, n_steps=None, with_atoms=False,
           valence_check=False, exact=False, similarity=False, train_library=None, patterns=None, pattern_options=None, huckel=False,
           ppp=False, ppp_cis=False, aromaticity=False, ring_currents=False, cluster_threshold=None, diverse=None, reactivity=False,
           ppp_dscf=False, ppp_scf=None):
    """generation_guidance.py:83-184: sample with guidance, check stability, evaluate the target and the predicted
    properties at t=0, rank all / stable molecules by target value.  Returns a dict instead of plotting.  n_steps: reverse
    steps per molecule (None: all T).  with_atoms: also convert every molecule to its graph of atoms (gaudi_amd.gor2goa, hydrogens
    placed) and add ``atoms`` (one record per molecule), ``fingerprints`` and ``mol_unique`` to the dict.  valence_check (with
    with_atoms): every record also carries its bond orders and formal charges (gaudi_amd.gor2goa.bond_orders), and the dict gains
    ``mol_valid`` (built with a valence-checked structure / all), ``valid`` (one bool per molecule) and ``best_valid`` (the
    ranking restricted to the valid molecules, as ``best_stable`` is to the stable ones).  The set of keys with_atoms alone
    returns is kept as it was.  exact (with with_atoms): every record is numbered canonically (gaudi_amd.gor2goa.canonical),
    ``mol_unique`` counts ``canon_keys`` (added: one per molecule, None where not built, ``("fp", fingerprint)`` where the
    search gave up) instead of fingerprints, and with valence_check the dict gains ``smiles``.  similarity (with with_atoms): the
    dict gains ``diversity`` -- what a stronger guidance scale costs when the batch collapses onto a few skeletons -- and, with
    ``train_library`` (a gaudi_amd.similarity.Library on the model's engine), ``nearest_train_similarity`` and
    ``nearest_train_index`` per molecule, as analyze_atoms_for_molecules returns them.  patterns (with with_atoms): a list of
    patterns for gaudi_amd.substructure.search (``pattern_options``: its ``hydrogens`` / ``closed``), and the dict gains
    ``contains`` bool [B,P] -- which designed molecules hold which motif, False where the molecule was not built.  With
    ``patterns=None`` no search is launched.  huckel (with with_atoms): one more call (gaudi_amd.huckel.gap)
    and the dict gains ``huckel_gap`` float64 [B], the Hueckel HOMO-LUMO gap of every molecule in |beta| next to the predictor's
    values (NaN where the molecule was not built or not solved).  With ``huckel=False`` nothing is launched.  ppp (with with_atoms):
    one more call (gaudi_amd.ppp.frontier) and the dict gains ``ppp_gap``, ``ppp_ip`` and ``ppp_ea`` float64
    [B]: the PPP HOMO-LUMO gap and the Koopmans ionisation potential and electron affinity of every molecule in eV, on its built
    geometry (NaN where the molecule was not built or not solved).  With ``ppp=False`` nothing is launched.  ppp_cis (with
    with_atoms): the CIS stage on that ground state (gaudi_amd.ppp.optical; with ``ppp`` the same call) and
    the dict gains ``ppp_s1``, ``ppp_t1`` and ``ppp_bright`` float64 [B]: the lowest singlet, the lowest triplet and the lowest
    singlet with f >= 0.01 in eV (NaN where nothing was solved).  With ``ppp_cis=False`` nothing is launched.  aromaticity (with
    with_atoms): one more launch (gaudi_amd.aromaticity) and the dict gains ``kekule_count`` and ``clar``
    int64 [B]: the number of Kekule structures and the Clar number of every molecule (0 where the molecule was not built or not
    counted).  With ``aromaticity=False`` nothing is launched.  ring_currents (with with_atoms): one more call
    (gaudi_amd.aromaticity.ring_current_extremes) and the dict gains ``ring_current_max`` and
    ``ring_current_min`` float64 [B]: the extreme Hueckel-London ring currents of every molecule in units of benzene's, on its built
    geometry (NaN where the molecule was not built or not solved).  With ``ring_currents=False`` nothing is launched.
    reactivity (with with_atoms): one more call (gaudi_amd.reactivity.most_reactive without the ortho solves)
    and the dict gains ``min_para_localization`` and ``min_atom_localization`` float64 [B]: the smallest para-localization energy
    over the six-rings and the smallest radical localization energy over the centres that carry a hydrogen, in |beta| (NaN where
    the molecule was not built or not solved).  With ``reactivity=False`` nothing is launched.
    ppp_dscf (with with_atoms): one more call (gaudi_amd.ppp.ionization) and the dict gains ``ppp_ip_dscf`` and
    ``ppp_ea_dscf`` float64 [B]: the delta-SCF ionisation potential and electron affinity of every molecule in eV -- orbital
    relaxation included, next to the Koopmans ``ppp_ip`` / ``ppp_ea`` (NaN where the molecule was not built or a state was not
    solved).  With ``ppp_dscf=False`` nothing is launched.
    ppp_scf: "diis" sends what ``ppp`` and ``ppp_dscf`` compute to gaudi_ppp_scf (Pulay's DIIS) -- more rows
    solved, the same keys; absent or "damped": what it was.  design_sweep and refine take it too.
    cluster_threshold (with with_atoms and similarity): Butina clusters of the built molecules at that similarity
    (gaudi_amd.similarity.cluster), and the dict gains ``n_clusters`` and ``largest_cluster_fraction`` =
    the largest cluster / built molecules -- whether the batch collapsed onto a few skeletons, which the one mean ``diversity``
    does not show.  diverse (with with_atoms and similarity): the dict gains ``diverse_indices``, up to ``diverse`` MaxMin picks
    (gaudi_amd.similarity.pick_diverse) among the built molecules, as indices into the batch in pick order: the ones to take on.
    With ``cluster_threshold=None`` / ``diverse=None`` nothing is launched."""
    model.eval()
    cond_predictor.eval()
    nodesxsample = np.array([n_nodes] * args.batch_size, dtype=np.int64)
    start_time = time()
    x, one_hot, node_mask, edge_mask = sample_guidance(args, model, target_function, nodesxsample, scale=scale,
                                                       **({} if n_steps is None else dict(n_steps=n_steps)))
    seconds = time() - start_time
    print(f"Generated {x.shape[0]} molecules in {seconds:.2f} seconds")
    return _evaluate(args, model, cond_predictor, target_function, prop_dist, scale, x, one_hot, node_mask, edge_mask, seconds,
                     with_atoms, valence_check, exact, similarity, train_library, patterns, pattern_options, huckel, ppp, ppp_cis, aromaticity, ring_currents,
                     cluster_threshold=cluster_threshold, diverse=diverse, reactivity=reactivity, ppp_dscf=ppp_dscf, ppp_scf=ppp_scf)


def design_sweep(args, model, cond_predictor, targets_or_scales, nodes_dist, prop_dist, n_nodes, target=None, scale=1.0,
                 n_steps=None, with_atoms=False, valence_check=False, similarity=False, train_library=None, patterns=None,
                 pattern_options=None, huckel=False, ppp=False, ppp_cis=False, aromaticity=False, ring_currents=False,
                 cluster_threshold=None, diverse=None, reactivity=False, ppp_dscf=False, ppp_scf=None):
    """A sweep of the guidance strength and / or the aimed-at values in ONE sampling call: setting j runs on molecules
    j * batch_size .. (j + 1) * batch_size of a single batch whose value-target parameters differ per molecule
    (gaudi_sample_target), so the chip is filled once instead of len(settings) times.

    targets_or_scales: a list whose entries are numbers (guidance scales of ``target``, a ValueTarget with shared arrays) or
    ValueTargets with shared ([K]) arrays (each with its own centres / curvatures / scale; ``scale`` multiplies them all).
    The guidance window is one per call: settings whose windows differ are refused.  Returns one design()-shaped dict per setting, evaluated
    as design() does; ``seconds`` is the ONE call's time, ``molecules_per_second`` the whole call's rate.  similarity /
    train_library: as design takes them; every setting gets its own ``diversity``.  patterns / pattern_options: as design takes
    them; every setting gets its own ``contains``.  huckel: as design takes it; every setting gets its own ``huckel_gap``.
    ppp: as design takes it; every setting gets its own ``ppp_gap``, ``ppp_ip`` and ``ppp_ea``.  ppp_cis: as design takes it; every
    setting gets its own ``ppp_s1``, ``ppp_t1`` and ``ppp_bright``.  aromaticity: as design takes it; every setting gets its own
    ``kekule_count`` and ``clar``.  ring_currents: as design takes it; every setting gets its own ``ring_current_max`` and
    ``ring_current_min``.  reactivity: as design takes it; every setting gets its own ``min_para_localization`` and
    ``min_atom_localization``.  ppp_dscf: as design takes it; every setting gets its own ``ppp_ip_dscf`` and ``ppp_ea_dscf``.
    cluster_threshold / diverse: as design takes them; every setting gets its own ``n_clusters``,
    ``largest_cluster_fraction`` and ``diverse_indices`` (indices into the setting's own molecules)."""
    from .models_edm import ValueTarget
    model.eval()
    cond_predictor.eval()
    settings = []
    for s in targets_or_scales:
        if isinstance(s, ValueTarget):
            settings.append((s, 1.0))
        else:
            if not isinstance(target, ValueTarget):
                raise ValueError("a sweep over scales needs target= (a ValueTarget with shared arrays)")
            settings.append((target, float(s)))
    if not settings:
        raise ValueError("design_sweep needs at least one setting")
    if any(t.window != settings[0][0].window for t, _ in settings):
        raise ValueError("design_sweep runs one call, and a call has one guidance window: the settings' windows differ")
    bs, K = int(args.batch_size), int(cond_predictor.engine.K)

    def rows(name, fill, dtype):
        out = []
        for t, _ in settings:
            a = getattr(t, name)
            a = np.full(K, fill, dtype) if a is None else np.asarray(a, dtype)
            if a.shape != (K,):
                raise ValueError(f"design_sweep takes ValueTargets with shared [K] arrays, got {name} of shape {a.shape}")
            out.append(np.broadcast_to(a, (bs, K)))
        return np.concatenate(out, 0)

    scales = []
    for t, mult in settings:
        sc = np.float32(1.0) if t.scale is None else np.asarray(t.scale, np.float32)
        if np.ndim(sc):
            raise ValueError("design_sweep takes ValueTargets with a scalar scale")
        # (the strength design(..., scale=scale * mult) would give this setting: its own scale times the call's, ValueTarget.spec)
        scales.append(np.full(bs, np.float32(sc) * np.float32(float(scale) * mult), np.float32))
    mixed = ValueTarget(cond_predictor, rows("weights", 0, np.float32), rows("curvature", 0, np.float32),
                        rows("center", 0, np.float32), rows("side", 0, np.int32), np.concatenate(scales),
                        settings[0][0].window, name="sweep")
    nodesxsample = np.array([n_nodes] * (bs * len(settings)), dtype=np.int64)
    start_time = time()
    x, one_hot, node_mask, edge_mask = sample_guidance(args, model, mixed, nodesxsample, scale=1.0,
                                                       **({} if n_steps is None else dict(n_steps=n_steps)))
    seconds = time() - start_time
    print(f"Generated {x.shape[0]} molecules ({len(settings)} settings) in {seconds:.2f} seconds")
    N = x.shape[1]
    em = edge_mask.reshape(len(nodesxsample), N * N)
    out = []
    for j, (t, mult) in enumerate(settings):
        lo, hi = j * bs, (j + 1) * bs
        d = _evaluate(args, model, cond_predictor, t, prop_dist, float(scale) * mult, x[lo:hi], one_hot[lo:hi], node_mask[lo:hi],
                      em[lo:hi].reshape(-1, 1), seconds, with_atoms, valence_check, False, similarity, train_library, patterns,
                      pattern_options, huckel, ppp, ppp_cis, aromaticity, ring_currents, cluster_threshold=cluster_threshold,
                      diverse=diverse, reactivity=reactivity, ppp_dscf=ppp_dscf, ppp_scf=ppp_scf)
        d["molecules_per_second"] = x.shape[0] / seconds
        out.append(d)
    return out


def refine(args, model, cond_predictor, target_function, x, one_hot, node_mask, edge_mask, t_start, scale, n_steps=None,
           prop_dist=None, with_atoms=False, valence_check=False, similarity=False, patterns=None, pattern_options=None,
           huckel=False, ppp=False, ppp_cis=False, aromaticity=False, ring_currents=False, diverse=None, reactivity=False, ppp_dscf=False, ppp_scf=None):
    """Guided refinement of given molecules: noise them to time index t_start and run the guided reverse process from there
    (GaudiModel.refine), then evaluate as design does.  Returns design's dict plus ``seed_target_function_values``, the target
    of the molecules that went in, so the caller sees what the refinement bought.  similarity (with with_atoms): the seeds go
    through rings_to_atoms as well, and the dict gains ``diversity`` and ``similarity_to_seed`` [B], the similarity of every
    refined molecule with its own seed (0.0 where either was not built): how far the refinement moved.  patterns /
    pattern_options: as design takes them, on the refined molecules.  huckel, ppp, ppp_cis, aromaticity, ring_currents, reactivity, ppp_dscf: as design takes them, on
    the refined molecules.  diverse: as design takes it, on the refined molecules."""
    model.eval()
    cond_predictor.eval()
    bs, n_nodes = _to_numpy(x).shape[0], _to_numpy(x).shape[1]
    nm = _to_numpy(node_mask).astype(np.float32).reshape(bs, n_nodes, 1)
    em = _to_numpy(edge_mask).astype(np.float32).reshape(-1, 1)
    seed_vals = _to_numpy(get_target_function_values(_like_ref(_to_numpy(x).astype(np.float32)), _like_ref(_to_numpy(one_hot).astype(np.float32)),
                                                     target_function, nm, em, model))
    start_time = time()
    xr, h = model.refine(x, one_hot, nm, em, t_start, target_function=target_function, scale=scale, n_steps=n_steps)
    seconds = time() - start_time
    print(f"Refined {bs} molecules in {seconds:.2f} seconds")
    out = _evaluate(args, model, cond_predictor, target_function, prop_dist, scale, xr, h["categorical"], _like_ref(nm), _like_ref(em),
                    seconds, with_atoms, valence_check, False, similarity, None, patterns, pattern_options, huckel, ppp, ppp_cis, aromaticity, ring_currents,
                    diverse=diverse, reactivity=reactivity, ppp_dscf=ppp_dscf, ppp_scf=ppp_scf)
    out["seed_target_function_values"] = _like_ref(seed_vals)
    if similarity:
        from .similarity import fingerprints, rowwise_similarity
        seeds = _atoms(_like_ref(_to_numpy(x).astype(np.float32)), _like_ref(_to_numpy(one_hot).astype(np.float32)), _like_ref(nm),
                       args.dataset, model.engine)["atoms"]
        fps = [fingerprints(recs, args.dataset, engine=model.engine)["fp"] for recs in (seeds, out["atoms"])]
        out["similarity_to_seed"] = rowwise_similarity(fps[0], fps[1])
    return out


def _atoms(x, one_hot, node_mask, dataset, engine, valence_check=False, exact=False, similarity=False, train_library=None,
           patterns=None, pattern_options=None, huckel=False, ppp=False, ppp_cis=False, aromaticity=False, ring_currents=False,
           cluster_threshold=None, diverse=None, reactivity=False, ppp_dscf=False, ppp_scf=None):
    """The graph of atoms of every molecule (hydrogens placed, fingerprints; with valence_check bond orders and charges too): what
    the reference's eval_stability gets from gor2goa + xyz2mol + RDKit (generation_guidance.py:69-80), as far as it goes without
    RDKit."""
    from .gor2goa import rings_to_atoms
    atom_type = one_hot.argmax(2)
    keep = [node_mask[i, :, 0].bool() for i in range(x.shape[0])]
    recs = rings_to_atoms([(x[i][keep[i]], atom_type[i][keep[i]]) for i in range(x.shape[0])], dataset, place_hydrogens=True,
                          fingerprint=True, engine=engine, bond_orders=valence_check, **({"canonical": True} if exact else {}))
    keys = [r["fingerprint"] for r in recs]
    ids = keys
    if exact:
        ids = [None if r["status"] else r["canon_key"] if r["canon_key"] is not None else ("fp", r["fingerprint"]) for r in recs]
    built = [k for r, k in zip(recs, ids) if r["status"] == 0]
    out = dict(atoms=recs, fingerprints=keys, mol_unique=len(set(built)) / float(len(built)) if built else 0.0)
    if exact:
        out["canon_keys"] = ids
        if valence_check:
            from .gor2goa import smiles
            out["smiles"] = [smiles(r, dataset) for r in recs]
    if valence_check:
        out["valid"] = np.array([r["status"] == 0 and r["kekule_status"] == 0 for r in recs], dtype=bool)
        out["mol_valid"] = float(out["valid"].mean())
    if similarity:
        from .analyze import _similarity
        out.update(_similarity(recs, [r["status"] == 0 for r in recs], dataset, engine, train_library, cluster_threshold, diverse))
    if patterns is not None:
        from .substructure import search
        out["contains"] = search(recs, patterns, dataset, engine=engine, **(pattern_options or {}))["hit"]
    if huckel:
        from .huckel import gap
        out["huckel_gap"] = gap(recs, dataset, engine=engine)
    if ppp and not ppp_cis:
        from .ppp import frontier
        out.update({"ppp_" + k: v for k, v in frontier(recs, dataset, engine=engine, scf=ppp_scf).items() if k in ("gap", "ip", "ea")})
    if ppp_cis:
        from .ppp import summary_fields
        out.update(summary_fields(recs, dataset, engine=engine, ppp=bool(ppp), scf=ppp_scf))
    if aromaticity:
        from .aromaticity import summary_fields as resonance_summary
        out.update(resonance_summary(recs, dataset, engine=engine))
    if ring_currents:
        from .aromaticity import ring_current_extremes
        ext = ring_current_extremes(recs, dataset, engine=engine)
        out.update(ring_current_max=ext["ring_current_max"], ring_current_min=ext["ring_current_min"])
    if reactivity:
        from .reactivity import most_reactive
        ext = most_reactive(recs, dataset, bonds=False, engine=engine)
        out.update(min_para_localization=ext["min_para_localization"], min_atom_localization=ext["min_atom_localization"])
    if ppp_dscf:
        from .ppp import dscf_fields
        ext = dscf_fields(recs, dataset, engine=engine, scf=ppp_scf)
        out.update(ppp_ip_dscf=ext["ppp_ip_dscf"], ppp_ea_dscf=ext["ppp_ea_dscf"])
    return out


def _evaluate(args, model, cond_predictor, target_function, prop_dist, scale, x, one_hot, node_mask, edge_mask, seconds,
              with_atoms=False, valence_check=False, exact=False, similarity=False, train_library=None, patterns=None,
              pattern_options=None, huckel=False, ppp=False, ppp_cis=False, aromaticity=False, ring_currents=False,
              cluster_threshold=None, diverse=None, reactivity=False, ppp_dscf=False, ppp_scf=None):
    """The part of design after sampling (generation_guidance.py:96-184)."""
    if patterns is not None and not with_atoms:
        raise ValueError("patterns need with_atoms=True")
    if huckel and not with_atoms:
        raise ValueError("huckel needs with_atoms=True")
    if ppp and not with_atoms:
        raise ValueError("ppp needs with_atoms=True")
    if ppp_cis and not with_atoms:
        raise ValueError("ppp_cis needs with_atoms=True")
    if aromaticity and not with_atoms:
        raise ValueError("aromaticity needs with_atoms=True")
    if ring_currents and not with_atoms:
        raise ValueError("ring_currents needs with_atoms=True")
    if reactivity and not with_atoms:
        raise ValueError("reactivity needs with_atoms=True")
    if ppp_dscf and not with_atoms:
        raise ValueError("ppp_dscf needs with_atoms=True")
    if (similarity or train_library is not None) and not with_atoms:
        raise ValueError("similarity / train_library need with_atoms=True")
    if train_library is not None and not similarity:
        raise ValueError("train_library needs similarity=True")
    if (cluster_threshold is not None or diverse is not None) and not (with_atoms and similarity):
        raise ValueError("cluster_threshold / diverse need with_atoms=True and similarity=True")
    _check(x, node_mask)
    stability_dict, _, _, _, _ = eval_stability(x, one_hot, node_mask, edge_mask, dataset=args.dataset,
                                                engine=model.engine)
    print(f"{scale=}")
    print(f"{stability_dict['mol_stable']=:.2%} out of {x.shape[0]}")
    tvals = _to_numpy(get_target_function_values(x, one_hot, target_function, node_mask, edge_mask, model))
    pred = _to_numpy(predict(cond_predictor, x, one_hot, node_mask, edge_mask, model))
    if prop_dist is not None:
        pred = prop_dist.unnormalize(pred)
    print(f"Mean target function value: {tvals.mean():.4f}")
    order = np.argsort(tvals)  # best (lowest energy) first, as the reference's ranking
    stable = np.array(stability_dict["molecule_stable_bool"], dtype=bool)
    if stable.any():
        print(f"Mean target function value (from stable): {tvals[stable].mean():.4f}")
    out = dict(stability=stability_dict, best_stable=order[stable[order]], x=x, one_hot=one_hot, node_mask=node_mask, edge_mask=edge_mask, target_function_values=_like_ref(tvals),
               pred=_like_ref(pred), best=order, seconds=seconds, molecules_per_second=x.shape[0] / seconds)
    if with_atoms:
        out.update(_atoms(x, one_hot, node_mask, args.dataset, model.engine, valence_check, exact, similarity, train_library,
                          patterns, pattern_options, huckel, ppp, ppp_cis, aromaticity, ring_currents, cluster_threshold, diverse,
                          reactivity, ppp_dscf, ppp_scf))
        print(f"{out['mol_unique']=:.2%} of the built molecules")
        if valence_check:
            out["best_valid"] = order[out["valid"][order]]
            print(f"{out['mol_valid']=:.2%} out of {x.shape[0]}")
    return out


def main(args, cond_predictor_args, prop_mean=None, prop_std=None, target="max_gap", batch_size=512, scale=0.6,
         n_nodes=10, device=0):
    """generation_guidance.main (reference lines 187-222) for checkpoint directories in the reference's format.

    ``args`` / ``cond_predictor_args`` come from ``gaudi_amd.checkpoint.get_edm_args / get_cond_predictor_args``
    (``args.txt`` + ``model.pt``).  The reference builds a dataloader only to obtain the property normalisation
    (``mean`` / ``std``, models_edm.py:111-112), which is not stored in checkpoints: pass it explicitly.  ``target`` is
    "max_gap" or "opv" (the two targets shipped with the reference) or a LinearTarget factory taking the predictor."""
    from .models_edm import (PropertyNorm, get_cond_predictor_model, get_model, target_function_max_gap,
                             target_function_opv)
    args.batch_size = batch_size  # the reference hard-codes these three knobs in main()
    model, nodes_dist, _ = get_model(args, device=device)
    cond_predictor = get_cond_predictor_model(cond_predictor_args, model=model)
    prop_dist = None
    if prop_mean is not None:
        prop_dist = PropertyNorm(prop_mean, prop_std)
    if target == "max_gap":
        target_function = target_function_max_gap(cond_predictor)
    elif target == "opv":
        if prop_dist is None:
            raise ValueError("the OPV target needs the property mean/std (prop_dist.unnormalize)")
        target_function = target_function_opv(cond_predictor, prop_dist)
    else:
        target_function = target(cond_predictor)
    return design(args, model, cond_predictor, target_function, nodes_dist, prop_dist, scale, n_nodes)
