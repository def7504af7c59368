"""Worker of test_eval_report.py::test_two_gloo_ranks_hold_the_single_process_report: one gloo rank scores its shard of a 711-row
logit table with evalcount.accumulate_report, all-reduces state and report as ONE fp64 vector (what CaraEngine.evaluate(report=True)
does with the kernel's words) and saves it."""
import os

import torch
import torch.distributed as dist

ROWS, CLASSES, BINS, BATCH, SEED = 711, 37, 15, 256, 8


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from cara_amd import evalcount as EC
    from cara_amd.dist import allreduce_sum_, eval_shard
    from tests.test_eval_shard import table
    logits, labels = table(CLASSES, ROWS, seed=SEED)
    st, rep = EC.new_state(), EC.new_report(CLASSES, BINS)
    mine = eval_shard(ROWS, rank, world, BATCH)
    for i in range(mine.start, mine.stop, BATCH):
        j = min(i + BATCH, mine.stop)
        pad = BATCH - (j - i)   # (the padded form of ResidentSplit.eval_shard: BATCH rows, n_valid of them real)
        lg = torch.cat([logits[i:j], logits[i:i + 1].expand(pad, -1)])
        lb = torch.cat([labels[i:j], labels[i:i + 1].expand(pad)])
        EC.accumulate_report(st, rep, lg, lb, j - i)
    vec = torch.cat([st, EC.report_vector(rep)])
    allreduce_sum_(vec)
    torch.save(vec.clone(), out + f".{rank}")
    dist.destroy_process_group()
