"""Child process of test_two_ranks_on_one_gpu_stay_identical_with_one_all_reduce_per_step: rank `argv[1]` of `argv[2]`, every rank on
cuda:0 over gloo.  Two SAM steps of the depth-2, 32-pixel model on this rank's own rows of the synthetic split, with its own DropPath
multipliers; writes the trainable tensors before and after, AdamW's moments, the losses, the SAM state of every step and the number of
all-reduces the steps issued to `argv[3]`.<rank>.pt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

STEPS, RHO = 2, 0.05
ROWS = ([[7, 0, 3, 11], [2, 9, 5, 1]], [[4, 4, 10, 6], [8, 1, 0, 3]])      # [rank][step]


def main():
    rank, world, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from cara_amd import dist as cdist
    from cara_amd.optim import AdamW
    from tests import test_augmented_feed_gpu as A
    from tests.test_mix_gpu import _dp
    calls = []
    real = cdist.allreduce_sum_
    cdist.allreduce_sum_ = lambda flat, group=None: (calls.append(flat.numel()), real(flat, group))[1]
    m = A._model("bf16").train()
    eng = m._cara_engine
    split = A._split()
    start = {n: p.detach().cpu().clone() for n, p in A._trainable(m).items()}
    opt = AdamW(eng.trainable_parameters(), lr=1e-3, weight_decay=1e-4)
    losses, norms = [], []
    for it in range(STEPS):
        rows = torch.tensor(ROWS[rank][it], device="cuda")
        boxes = A._same_size_boxes(A.BATCH, seed=10 * rank + it).cuda()
        losses.append(float(eng.train_step_resident(split, rows, opt, droppath=_dp(20 + 2 * it + rank), boxes=boxes, clip_grad=1.0, sam_rho=RHO)))
        norms.append(eng.sam_norm.tolist())
    assert eng.resident_bad_rows() == 0
    torch.save({"start": start, "params": {n: p.cpu() for n, p in A._trainable(m).items()},
                "moments": [t.cpu() for p in eng.trainable_parameters() for t in (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])],
                "losses": losses, "sam_norm": norms, "allreduces": len(calls), "steps": STEPS}, f"{out}.{rank}.pt")
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
