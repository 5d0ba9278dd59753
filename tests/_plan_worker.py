"""Child process of tests/test_gpu_plan_matrix.py.  The library reads its DP_* plan knobs once per process, so every
knob setting of the matrix runs this script in a fresh process (under the kernel trace):

    python tests/_plan_worker.py REPORT.json [--loose NAME,NAME,...] CASE [CASE ...]

For each case: one eager forward + loss + backward of SoftPoolingGcnEncoder, checked against the CPU oracle the way
tests/test_gpu_model.py checks it — the forward against the oracle's own arg-max, then the forward, assign_tensor, the
loss and every parameter gradient with the HIP forward's max-readout winners forced into the oracle (tests/parity.py).
For `enz` also: an evaluation forward (torch.no_grad()) must equal the training forward bit for bit, and a forward +
loss + backward captured in a hipGraph must replay to the eager step's bits, with the same inputs and with new inputs
written in place.  Tensors named by --loose are float-atomic sums under the plan being tested: those are compared at
rtol 1e-5 / atol 1e-7 instead.  For `mixed` the level-0 launch counters must read [1, 0]: the persistent forward with
the per-phase backward (a shape whose backward does not fit the persistent kernel's LDS block, l0b_geometry).

Before each case the worker drains the stream and launches torch.cuda._sleep as a marker, so that the parent can split
the kernel trace per case.  REPORT.json: {"ok": bool, "cases": [{"name", "ok", "error", "seconds"}]}."""
import ctypes as C
import json
import os
import sys
import time
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_pooling_amd import _lib                                        # noqa: E402
from graph_pooling_amd.encoders import SoftPoolingGcnEncoder              # noqa: E402
from oracle import diffpool_oracle as O                                   # noqa: E402
from tests.parity import _oracle_run, close, grads_close, gpu_winners     # noqa: E402

# name: (B, N, F, H, C), assign ratio, edge probability, link loss, and what differs from the defaults below
CASES = {
    "enz": dict(shape=(20, 100, 3, 20, 6), ratio=0.1, p=0.10, link=True),
    "dd": dict(shape=(20, 500, 89, 20, 2), ratio=0.1, p=0.02, link=False),
    "odd": dict(shape=(5, 67, 11, 12, 3), ratio=0.25, p=0.15, link=True),
    "widek": dict(shape=(3, 256, 16, 20, 3), ratio=0.6, p=0.05, link=True),
    # test_multi_pool_against_oracle_PARITY_UNPINNED
    "p2": dict(shape=(4, 64, 6, 10, 3), ratio=0.25, p=0.1, link=True, P=2, n_min=8, seed=5, pseed=6),
    # test_er_two_level_pooling_against_oracle_PARITY_UNPINNED
    "er4": dict(shape=(4, 1024, 64, 20, 2), ratio=0.25, p=0.01, link=True, P=2, n_min=1024, onehot=False, seed=41,
                pseed=42),
    # the S-ER shape at B = 16: enough 128 x 128 tiles for the split-bf16 GEMM (er4 has too few)
    "er16": dict(shape=(16, 1024, 64, 20, 2), ratio=0.25, p=0.01, link=True, P=2, n_min=1024, onehot=False, seed=41,
                 pseed=42),
    # B > 64: the per-phase level-0 plan without any knob; ceil(N / 32) * B >= 256 makes 32-row panel tiles the default
    "b66": dict(shape=(66, 128, 8, 12, 2), ratio=0.1, p=0.05, link=False),
    # K = 56 at N = 64: the forward takes 32-row blocks; the backward's staged rows, 2*32*K + 32*D + K^2 = 8640 floats
    # (D = 60), exceed the block's 8320, so only the backward falls back
    "mixed": dict(shape=(4, 64, 5, 20, 3), ratio=0.875, p=0.15, link=False),
}
MARKER_CYCLES = 1000


def _batch(c, seed):
    B, N, F_, H, Cc = c["shape"]
    return O.make_batch(B, N, F_, n_min=c.get("n_min", max(1, N // 10)), p=c["p"], seed=seed, n_classes=Cc,
                        onehot=c.get("onehot", True))


def _same(what, a, b, loose):
    a, b = a.detach().cpu(), b.detach().cpu()
    if what in loose:
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7, msg=lambda m: f"{what}: {m}")
    elif not torch.equal(a, b):
        d = float((a.double() - b.double()).abs().max()) if a.shape == b.shape else float("nan")
        raise AssertionError(f"{what}: not bit-identical (max |diff| {d:.3e})")


def _level0_counts(lib):
    out = []
    for which in (0, 1):
        us, n = C.c_double(0.0), C.c_int(0)
        _lib.check(lib.dp_profile_level0_read(which, C.byref(us), C.byref(n)))
        out.append(n.value)
    return out


def run_case(name, loose, lib):
    c = CASES[name]
    B, N, F_, H, Cc = c["shape"]
    P, link = c.get("P", 1), c["link"]
    x, adj, nn_, label = _batch(c, c.get("seed", 1))
    model = SoftPoolingGcnEncoder(N, F_, H, H, Cc, 3, H, assign_ratio=c["ratio"], num_pooling=P, linkpred=link)
    params = O.init_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=c.get("pseed", 0),
                           bias_scale=0.1)
    model.load_state_dict(params)
    model = model.cuda()
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    counted = name == "mixed"
    if counted:
        _lib.check(lib.dp_profile_level0(1))
    ypred = model(xd, ad, nn_, assign_x=xd)
    win = gpu_winners(model, P + 1)
    loss = model.loss(ypred, ld, ad, nn_) if link else model.loss(ypred, ld)
    loss.backward()
    torch.cuda.synchronize()
    if counted:
        n = _level0_counts(lib)
        _lib.check(lib.dp_profile_level0(0))
        assert n == [1, 0], f"level-0 kernels launched {n} times (forward, backward): not the mixed plan"
    close(ypred, O.softpool_forward(params, x, adj, nn_, x, num_pooling=P)[0])     # the oracle's own arg-max
    yo, inter, lo, go = _oracle_run(params, x, adj, nn_, label, link, num_pooling=P, winners=win)
    close(ypred, yo)
    close(model.assign_tensor, inter["assign_0"], 1e-4, 1e-6)
    close(loss, lo, 1e-4, 1e-6)
    grads_close(model, go)
    if name == "enz":
        y_train = ypred.detach().clone()
        del ypred, loss                                  # (their autograd graph holds the parameters' grad nodes)
        with torch.no_grad():
            y_eval = model(xd, ad, nn_, assign_x=xd)
        _same("eval ypred", y_eval, y_train, ())
        # the capture on a model of its own: grad-accumulation nodes of an earlier eager step must not be alive
        # while the backward is captured (they would run on the stream they were created on)
        cap = SoftPoolingGcnEncoder(N, F_, H, H, Cc, 3, H, assign_ratio=c["ratio"], num_pooling=P, linkpred=link)
        cap.load_state_dict(params)
        _replay(cap.cuda(), c, loose)


def _replay(model, c, loose):
    """A captured step against the eager step (test_step_is_capturable_in_a_hip_graph_and_replays_bit_identically)."""
    link = c["link"]
    x, adj, nn_, label = _batch(c, c.get("seed", 1))
    xd, ad, ld = x.cuda(), adj.cuda(), label.cuda()
    nd = torch.from_numpy(nn_).cuda()                    # device num_nodes: no H2D inside the captured region

    def step():
        model.zero_grad(set_to_none=True)
        y = model(xd, ad, nd, assign_x=xd)
        loss = model.loss(y, ld, ad, nd) if link else model.loss(y, ld)
        loss.backward()
        return y, loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    model.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        y_static, loss_static = step()
    grads_static = {k: p.grad for k, p in model.named_parameters()}
    for seed in (c.get("seed", 1), 9):                  # same inputs, then new inputs written in place
        x2, adj2, nn2, label2 = _batch(c, seed)
        xd.copy_(x2); ad.copy_(adj2); ld.copy_(label2); nd.copy_(torch.from_numpy(nn2))
        g.replay()
        torch.cuda.synchronize()
        y_g, loss_g = y_static.clone(), loss_static.clone()
        grads_g = {k: v.clone() for k, v in grads_static.items()}
        y_e, loss_e = step()                             # eager, same inputs
        torch.cuda.synchronize()
        _same(f"replay ypred (inputs {seed})", y_g, y_e, ())
        _same(f"replay loss (inputs {seed})", loss_g, loss_e, ())
        bad = []
        for k, p in model.named_parameters():
            try:
                _same(k, grads_g[k], p.grad, loose)
            except AssertionError as e:
                bad.append(str(e))
        assert not bad, f"replay gradients (inputs {seed}): " + "; ".join(bad)
    del g


def main():
    report, args = sys.argv[1], sys.argv[2:]
    loose = ()
    if args[:1] == ["--loose"]:
        loose, args = tuple(s for s in args[1].split(",") if s), args[2:]
    unknown = [a for a in args if a not in CASES]
    assert args and not unknown, f"unknown cases {unknown}; known: {sorted(CASES)}"
    lib = _lib.load()
    out = {"ok": True, "cases": []}
    for name in args:
        torch.cuda.synchronize()
        torch.cuda._sleep(MARKER_CYCLES)                 # the parent's per-case boundary in the kernel trace
        torch.cuda.synchronize()
        t0 = time.monotonic()
        rec = {"name": name, "ok": True, "error": ""}
        fatal = False
        try:
            run_case(name, loose, lib)
        except AssertionError as e:
            rec.update(ok=False, error=str(e)[-3000:])
        except Exception:                                # a library error: stop here, the process may be unusable
            rec.update(ok=False, error=traceback.format_exc()[-3000:])
            fatal = True
        torch.cuda.synchronize()
        rec["seconds"] = round(time.monotonic() - t0, 2)
        out["cases"].append(rec)
        out["ok"] = out["ok"] and rec["ok"]
        print(f"[plan-worker] {name}: {'ok' if rec['ok'] else 'FAILED'} ({rec['seconds']} s)", flush=True)
        if fatal:
            break
    with open(report, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
