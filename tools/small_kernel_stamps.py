"""Phase timing inside the pooled-level kernels (diagnostic build: DP_STAMP=1 graph_pooling_amd/csrc/build.sh, then
DP_LIB=graph_pooling_amd/libdiffpool_hip_stamp.so PYTHONPATH=. python tools/small_kernel_stamps.py).
Prints shader-clock deltas between the phase stamps of workgroup 0 of the LAST forward / backward small-level launch,
and those of the whole-level backward kernel (k_small_level_bwd, the one the DD step runs) with the prediction-head
backward folded in (run with DP_NO_HEAD_FOLD=1 for the kernel without it: its head prologue then reads 0)."""
import ctypes as C
import torch
import bench
from graph_pooling_amd import _lib

lib = _lib.load()
w = bench.WORKLOADS["dd"]
model, batch, _ = bench.make_model_and_batch(w, False, torch.device("cuda"))
for _ in range(5):
    model.zero_grad(set_to_none=True)
    y = model(batch["x"], batch["adj"], batch["nn"], assign_x=batch["x"])
    model.loss(y, batch["label"]).backward()
torch.cuda.synchronize()
buf = (C.c_ulonglong * 64)()
lib.dp_debug_stamps.restype = C.c_int
assert lib.dp_debug_stamps(buf) == 0
fw = [buf[i] for i in range(5)]
bw = [buf[32 + i] for i in range(8)]
names_f = ["stage+bn", "P=XW", "U=AP", "normalise"]
names_b = ["stage", "bn sums", "dU rows", "G=A^T dU (+P, db)", "dW", "dX", "dA'", "part2_prev"]
print("forward  (cycles):", {n: fw[i + 1] - fw[i] for i, n in enumerate(names_f)}, "total", fw[-1] - fw[0])
print("backward staging: issue", buf[32 + 8] - bw[0], "wait+barrier", buf[32 + 9] - buf[32 + 8], "bn sums", bw[1] - buf[32 + 9])
print("backward G phase: to-db-end", buf[32 + 10] - bw[2], "G tile", buf[32 + 11] - buf[32 + 10], "P (wave 0: none)", buf[32 + 12] - buf[32 + 11], "barrier wait", bw[3] - buf[32 + 12])
print("backward (cycles):", {n: bw[i + 1] - bw[i] for i, n in enumerate(names_b[:-1])}, "total", bw[-1] - bw[0])

# k_small_level_bwd: [1][16] entry, 17 burst issued, 18 burst landed, 19 head prologue done, 20 layers done (the kernel's
# last stamp: the head's dW / db are summed by the step's final launch, k_reduce_slabs_head)
lb = [buf[32 + i] for i in range(16, 21)]
if lb[0]:
    fold = lb[3] != 0
    print("level backward (cycles): issue", lb[1] - lb[0], "wait+barrier", lb[2] - lb[1],
          "head prologue", (lb[3] - lb[2]) if fold else 0, "layers", lb[4] - (lb[3] if fold else lb[2]),
          "total", lb[4] - lb[0])
