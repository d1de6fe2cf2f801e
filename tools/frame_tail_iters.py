"""Refinement lengths of the pairs the headline rotates through and of the 32 data seeds of full_solve_batched: LM iterations per solve
(rsdsfm_frame_result.refine_summary; on the radius-factorised path a solve of `it` iterations consumes it + 1 slots, tools/refine_slots.py)
as a histogram, and per pair in solve order -- what a rule that sizes the refinement's first chunk from the context's recent solves would
have had to go on.    usage (GPU box): python tools/frame_tail_iters.py [solves on the headline's pairs]"""
import collections
import sys

import torch

sys.path.insert(0, ".")
import rsdsfm

dev = torch.device("cuda", 0)
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 64


def run(seeds, steps, label):
    flows, meta = rsdsfm.synth.make_flow_sequence(5, seeds)
    rows, cols = meta["rows"], meta["cols"]
    imgs = [torch.from_numpy(f).to(dev) for f in flows]
    dm = torch.empty((cols, rows), dtype=torch.float64, device=dev)
    its = []
    with rsdsfm.Solver(0) as s:
        for i in range(steps):
            r = s.solve_frame_dev(imgs[i % len(imgs)].data_ptr(), rows, cols, meta["K"], meta["gamma"], dm.data_ptr(), trials=50, tol=0.05, seed=1 + i)
            its.append(r["refine_summary"]["num_iterations"])
    hist = collections.Counter(its)
    print("%s: %d solves, LM iterations -> solves: %s" % (label, steps, sorted(hist.items())))
    print("  in solve order: " + " ".join(str(x) for x in its))
    for j in range(min(len(imgs), 4)):
        print("  pair %d: %s" % (j, " ".join(str(x) for x in its[j::len(imgs)])))
    # what following the context's history would have cost: chunk = max of the last h solves' slots (+ a), against the fixed 7
    slots = [x + 1 for x in its]
    for h, a in ((1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (4, 1)):
        empty = second = 0
        for i in range(4, len(slots)):
            chunk = max(slots[i - h:i]) + a
            if slots[i] > chunk:
                second += 1
            else:
                empty += chunk - slots[i]
        print("  rule max(last %d)%s: passes that find the solve finished besides the closing one %.2f per solve, second chunks %d of %d" % (
            h, " + 1" if a else "", empty / (len(slots) - 4), second, len(slots) - 4))
    empty = sum(max(0, 7 - x) for x in slots[4:])
    second = sum(1 for x in slots[4:] if x > 7)
    print("  fixed 7 slots: %.2f per solve, second chunks %d of %d" % (empty / (len(slots) - 4), second, len(slots) - 4))


run([0x5EED0005 + 7919 * j for j in range(4)], steps, "headline pairs (bench.py full_solve: 4 data seeds in rotation, a new sampler seed per step)")
run([0x5EED0005 + 1000 * i for i in range(32)], 32, "full_solve_batched's 32 data seeds (one solve each, in order)")
