"""Worker for tests/test_gpu_value_target.py::test_two_ranks_per_sample_parameters: launched by torch.distributed.run (gloo)
with both ranks on GPU 0.  Each rank runs the REAL Engine on its contiguous shard of a batch whose value-target parameters
differ per molecule -- sample_sharded(per_sample=...) hands it its slice by global index -- then ONE all_gather; rank 0 also runs
the unsharded batch for the bit-for-bit comparison."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as dist  # noqa: E402

from gaudi_amd import dist as gdist  # noqa: E402
from gaudi_amd import synth  # noqa: E402
from gaudi_amd.engine import Engine  # noqa: E402
from gaudi_amd.sampling_edm import build_masks  # noqa: E402


def main():
    out_dir = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    T, seed, K = 20, 77, 5
    eargs = synth.edm_args(nf=32, n_layers=2, diffusion_steps=T)
    pargs = synth.pred_args(nf=36, n_layers=3)
    eng = Engine(0)
    eng.load_edm(eargs, synth.synth_edm_state_dict(eargs, 1, seed=11))
    eng.load_predictor(pargs, synth.synth_predictor_state_dict(pargs, 1, K, seed=12))
    eng.set_steps_per_launch(7)  # 20 steps = 2 full launches + one of 6
    nodes = np.array([5, 7, 3, 7, 6, 11, 2, 9, 11, 4, 8])  # global batch of 11 -> shards of 6 and 5, padded to N = 11
    nm3, em_flat, _ = build_masks(nodes, int(nodes.max()), False)
    B, N = nm3.shape[0], nm3.shape[1]
    nm, em = nm3.reshape(B, N), em_flat.reshape(B, N, N)
    rng = np.random.default_rng(3)
    shared = dict(w=np.array([0, -1, 0, 0, 0], np.float32), side=np.array([0, 1, -1, 1, 0], np.int32), window=(3, 18))
    per = dict(q=rng.uniform(0.2, 1.5, (B, K)).astype(np.float32), c=rng.standard_normal((B, K)).astype(np.float32),
               scale=rng.uniform(0.2, 2.0, B).astype(np.float32))

    def sample_fn(nm_s, em_s, offset, per_sample):
        x, h, _ = eng.sample_target(nm_s, em_s, dict(shared, **per_sample), seed=seed, sample_offset=offset)
        return x, h

    lo, hi, x, h = gdist.sample_sharded(sample_fn, nm, em, rank, world, engine=eng, per_sample=per)
    xs, hs = gdist.gather_to_all(x, h, B, N, 1)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), x=xs, h=hs, lo=lo, hi=hi)
    if rank == 0:
        x_full, h_full = sample_fn(nm, em, 0, per)
        x_uni, _ = sample_fn(nm, em, 0, {k: np.broadcast_to(v[:1], v.shape).copy() for k, v in per.items()})
        np.savez(os.path.join(out_dir, "unsharded.npz"), x=x_full, h=h_full, x_uniform=x_uni)
    eng.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        import traceback
        with open(os.path.join(sys.argv[1], f"err{os.environ.get('RANK', '0')}.txt"), "w") as f:
            f.write(traceback.format_exc())
        raise
