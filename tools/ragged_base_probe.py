"""One torch.profiler step of SparseBatchGcnEncoderGraph forward + loss + backward on a RAGGED batch (CsrBatch), kernels by
device time.  The batch of tools/csr_batch_probe.py: B = 20 graphs whose sizes are drawn with a fixed seed from 30..5748
(log-uniform, the largest pinned at DD's 5 748), degree ~10; F 16, hidden / embedding 32, three GraphConv layers,
pred_hidden_dims [50], GraphConv biases of scale 0.3 so the padded rows' constants are not zero.  No threshold: the output
(profiles/ragged_base_probe.txt) is the record for whoever tunes this path next.

    PYTHONPATH=. python tools/ragged_base_probe.py"""
import hashlib
import os
import re
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from csr_batch_probe import batch, sizes  # noqa: E402
from graph_pooling_amd import _lib  # noqa: E402
from graph_pooling_amd.sparse import SparseBatchGcnEncoderGraph  # noqa: E402


def main():
    torch.manual_seed(0)
    lp = _lib.LIB_PATH
    digest = hashlib.sha256(open(lp, "rb").read()).hexdigest()[:16]
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__} (HIP {torch.version.hip}); "
          f"library {os.path.basename(lp)} sha256 {digest}")
    F_, H, E = 16, 32, 32
    sz = sizes()
    g = batch(sz)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(g.n_total, F_, device="cuda", generator=gen)
    label = torch.arange(g.num_graphs, device="cuda") % 2
    for bn in (True, False):
        model = SparseBatchGcnEncoderGraph(F_, H, E, 2, 3, pred_hidden_dims=[50], bn=bn).cuda()
        with torch.no_grad():
            for m in model._stack_modules(model.conv_first, model.conv_block, model.conv_last):
                m.bias.copy_((torch.rand(m.bias.shape, device="cuda", generator=gen) * 2 - 1) * 0.3)

        def step():
            model.zero_grad(set_to_none=True)
            loss = model.loss(model(x, g), label)
            loss.backward()

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            step()
        e1.record()
        e1.synchronize()
        nb = torch.from_numpy(g.num_nodes).unsqueeze(1)
        won = [int((model.saved_activation(li, "readout_argmax").cpu() >= nb).sum()) for li in range(3)]
        print(f"B={g.num_graphs} sizes={sorted(sz.tolist())} n_total={g.n_total} nnz={int(g.indptr[-1])} F={F_} "
              f"hidden={H} embedding={E} bn={bn}; table rows {g.min_n}..{g.n_idx - 1}; readout entries won by a padded "
              f"row per layer: {won} of {g.num_graphs * H}: {e0.elapsed_time(e1) / 10:.3f} ms per step (10 steps, host "
              "launch time included)")
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        tot = {}
        for ev in prof.events():
            if ev.device_type == torch.autograd.DeviceType.CUDA:
                t = tot.setdefault(ev.name, [0.0, 0])
                t[0] += ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
                t[1] += 1
        total = sum(v[0] for v in tot.values())
        print(f"    device time of one profiled step: {total / 1e3:.3f} ms over {sum(v[1] for v in tot.values())} "
              "kernels; by time:")
        for name, (t, c) in sorted(tot.items(), key=lambda kv: -kv[1][0])[:18]:
            print(f"    {t / 1e3:8.3f} ms  {100 * t / max(total, 1e-9):5.1f} %  x{c}  {name[:110]}")
        mine = {n: v for n, v in tot.items() if any(k in n for k in ("k_ragged_padval", "k_suffix_", "k_segment_max_",
                                                                     "k_floor_", "k_bn_ragged_", "k_pad_const_", "k_readout_",
                                                                     "k_ragged_colsum"))}
        print("    the ragged readout's own kernels: " + "; ".join(
            f"{re.search(r'k_[a-z_0-9]+', n).group(0)} x{c} {t:.1f} us" for n, (t, c) in sorted(mine.items())))


if __name__ == "__main__":
    main()
