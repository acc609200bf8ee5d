#!/usr/bin/env python3
"""bench.py — images/sec of the full PraNet-V2 (Res2Net-50) training step at 352x352, bs=32 per GPU.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 8 ...          # starts 8 ranks itself (one per GPU, torch.distributed.run as a CHILD process) and exits with their status
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...   # the same ranks, launched by the caller

A step = forward + 4x structure loss + backward + clamp(0.5) + Adam(1e-4) [+ RCCL gradient all-reduce], i.e. everything the
reference runs between optimizer.zero_grad() and optimizer.step() (MyTrain_med.py:59-86), on synthetic data (images N(0,1),
1-3 random ellipses per mask) with random-init weights (the reference's default init, seed 0).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times --steps steps and prints the line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).
    --dump-outputs DIR   after the timed steps, rank 0 writes what the last timed step handed its caller as DIR/<name>.npy (float32; fixed,
                         seeded samples of the large arrays, 24 MB at most): loss.npy, logits.npy, weights.npy (see dump_outputs)
    --full               everything else the benchmark measures, after the headline, as extra objects of the same line:
  roofline     — the dominant kernel family (implicit-GEMM conv forward+dgrad on MFMA): algorithmic FLOPs / measured kernel
                 time, timed with HIP events on the launch stream inside an instrumented extra step.
  fp32, fp32fast, configs, module_surface[_verbatim], inference, dp1 — the other precisions / configurations (--no-fp32-line, --no-extras).
  cpu_baseline — the CPU oracle (oracle/pranet_oracle.py, a torch-CPU port of the same step) timed on this host's cores on a
                 bounded sample (rank 0, N=1 only; --no-cpu-baseline).
  dp.exposed_comm_ms — multi-rank runs: the step with the collectives minus the same graphs without them.
"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
os.environ.setdefault("PN2_NO_PRETRAINED", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0     # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
PEAK_F64_TFLOPS = 78.6      # v_mfma_f64_16x16x4_f64 (the fp32 parity path accumulates in double)
PEAK_HBM_GBS = 8000.0
TRAIN_GFLOP_PER_IMG = 78.02   # 13.004 GMAC fwd x 2 x 3 (fwd + dgrad + wgrad)


def synthetic(n, size, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((n, 3, size, size), generator=g)
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32), indexing="ij")
    m = torch.zeros((n, 1, size, size))
    for i in range(n):
        for _ in range(int(torch.randint(1, 4, (1,), generator=g))):
            cy, cx = (torch.rand(2, generator=g) * 0.6 + 0.2) * size
            ry, rx = (torch.rand(2, generator=g) * 0.16 + 0.08) * size
            m[i, 0][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1.0
    return x.to(device), m.to(device)


def cpu_baseline(size):
    """the CPU oracle (kind 'port': oracle/pranet_oracle.py, a torch-CPU restatement of the same step) on this host's cores, fp32:
    eval forward at bs=1 and bs=32 and one train step at bs=8 (extrapolated per image; bs=32 would take minutes), median after warm-ups.
    Bounded to ~20-30 s: bs=1 5 timed after 2 warm-ups; bs=32 eval and bs=8 train 3 timed after 1 warm-up."""
    import statistics
    from oracle import pranet_oracle as O
    from oracle import weights as W
    cores = min(os.cpu_count() or 1, 64)
    torch.set_num_threads(cores)
    P = W.make_state_dict(W.manifest_pranet_v2(1), seed=0)

    def med(fn, warm, reps):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return statistics.median(ts)
    x1, _ = W.synthetic_batch(1, size, seed=1234)
    x32, _ = W.synthetic_batch(32, size, seed=1234)
    x8, m8 = W.synthetic_batch(8, size, seed=1234)
    with torch.no_grad():
        t_e1 = med(lambda: O.pranet_v2_forward(O.clone_sd(P), x1, False), 2, 5)
        t_e32 = med(lambda: O.pranet_v2_forward(O.clone_sd(P), x32, False), 1, 3)
    st = {}
    t_tr = med(lambda: O.train_step(P, st, x8, m8), 1, 3)
    return {"value": round(8 / t_tr, 3), "unit": "images/sec", "cores": cores, "kind": "port",
            "eval_fwd_bs1_img_s": round(1 / t_e1, 2), "eval_fwd_bs32_img_s": round(32 / t_e32, 2), "train_bs8_s_per_step": round(t_tr, 3),
            "sample": f"oracle (torch CPU fp32, {cores} threads) at {size}x{size}: value = train step (fwd+4x structure_loss+bwd+clamp+Adam) at bs=8, median of 3 after 1 warm-up "
                      f"({t_tr:.2f} s/step; bs=32 extrapolates per image); eval forward bs=1 median of 5 after 2 warm-ups ({1e3 * t_e1:.0f} ms), bs=32 median of 3 after 1 ({t_e32:.2f} s)"}


def fp32_line(model_ctor, x, m, steps=5, mode="fp32"):
    """The same step with fp32 storage, eager + hipGraph.  mode "fp32": the parity path - conv contractions accumulated in double on v_mfma_f64_16x16x4_f64 (the
    precision all tight parity evidence is on, tests/test_gpu_parity.py); mode "fp32fast": fp32 products and sums on v_mfma_f32_16x16x4_f32 - the reference's own
    arithmetic (MyTrain_med.py runs without autocast) on the matrix pipe that is twice as fast (tests/test_gpu_bs32.py: literal 1e-4 on the conditioned fixture)."""
    import pn2
    from pn2.trainer import Trainer
    from pn2 import profile as prof
    pn2.set_compute_dtype(mode)
    torch.manual_seed(0)
    tr = Trainer(model_ctor(), lr=1e-4, clip=0.5)
    tr.capture(x, m, warmup=2)
    tr.replay(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.replay()
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / steps
    peak = PEAK_F32_TFLOPS if mode == "fp32fast" else PEAK_F64_TFLOPS
    out = {"value": round(x.shape[0] / el, 2), "unit": "images/sec", "ms_per_step": round(1e3 * el, 3), "steps": steps, "peak_tf": peak,
           "mfma_frac_whole_step": round(x.shape[0] / el * TRAIN_GFLOP_PER_IMG / 1e3 / peak, 4),
           "note": ("fp32 storage; fp32 products and sums on v_mfma_f32_16x16x4_f32 (157.3 TF/s dense peak), chains of 4 (forward / data gradient) or 8 (weight gradient) MFMAs met by round-to-nearest adds" if mode == "fp32fast" else
                    "fp32 storage; conv products / sums in double on v_mfma_f64_16x16x4_f64 (78.6 TF/s dense peak), one rounding per output")}
    try:          # the conv GEMM family of this mode against ITS matrix pipe (event-timed instrumented step, as the headline's roofline)
        r = prof.measure_step(tr, x, m, "fp32")["roofline"]
        tf = r["achieved"]
        out["roofline"] = {"kernel": "conv fwd+dgrad GEMMs (conv_gather_gemm<*>)", "bound": "mfma", "achieved": tf, "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                           "launches": r.get("launches"), "avg_launch_us": r.get("avg_launch_us")}
        if "wgrad" in r:
            out["roofline"]["wgrad"] = {"achieved": r["wgrad"]["achieved"], "frac": round(r["wgrad"]["achieved"] / peak, 4)}
    except Exception as e:          # noqa: BLE001
        out["roofline"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    pn2.set_compute_dtype("bf16")
    del tr
    torch.cuda.empty_cache()
    return out


def _timed_replay(tr, steps):
    tr.replay(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _config_roofline(tr, x, m):
    """The `roofline` object of a secondary configuration, measured like the headline's (pn2.profile.measure_step: HIP events around every launch of an
    instrumented eager step): the MFMA family (conv / Linear GEMMs forward + dgrad), the weight-gradient GEMMs and the six heaviest kernels."""
    from pn2 import profile as prof
    r = prof.measure_step(tr, x, m, "bf16")
    ro = r["roofline"]
    out = {k: ro[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "launches", "avg_launch_us") if k in ro}
    out["traffic"] = None
    if "wgrad" in ro:
        out["wgrad"] = {k: ro["wgrad"][k] for k in ("achieved", "frac", "launches")}
    if "per_launch_roofline" in ro:
        out["per_launch_roofline_frac"] = ro["per_launch_roofline"]["frac"]
    tot = sum(k["ms"] for k in r["kernels"].values())
    out["kernel_ms_total"] = round(tot, 3)
    out["top_kernels"] = {n: k for n, k in list(r["kernels"].items())[:6]}
    return out


def other_configs(dev, steps=10):
    """BASELINE configs 4 and 5 on this GPU (their single-GPU workloads), through the same fused Trainer + hipGraph replay as the headline."""
    import pn2
    from pn2.trainer import Trainer
    from lib.pranet import PVT_PraNet_V2
    from lib.networks import EMCADNet
    out = {}
    pn2.set_compute_dtype("bf16")
    torch.manual_seed(0)
    model = PVT_PraNet_V2(num_class=1).to(dev).train()
    tr = Trainer(model, lr=1e-4, clip=0.5)
    x, m = synthetic(16, 352, 1234, dev)
    tr.capture(x, m, warmup=2)
    el = _timed_replay(tr, steps)
    out["pvt_bs16_352"] = {"workload": "PVT-PraNet-V2 (pvt_v2_b2, DropPath 0.1) training step, bs=16 352x352 bf16 (config 4, one GPU)", "value": round(16 / el, 1),
                           "unit": "images/sec", "ms_per_step": round(1e3 * el, 3), "steps": steps,
                           "mfma_frac_whole_step": round(16 / el * 72.3 / 1e3 / PEAK_BF16_TFLOPS, 4)}       # 72.3 GFLOP per image and train step
    try:
        out["pvt_bs16_352"]["roofline"] = _config_roofline(tr, x, m)
    except Exception as e:          # noqa: BLE001
        out["pvt_bs16_352"]["roofline"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    del tr, model
    torch.cuda.empty_cache()
    torch.manual_seed(0)
    model = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, activation="relu6", encoder="pvt_v2_b2", pretrain=False, dual=True).to(dev).train()
    tr = Trainer(model, lr=1e-4, clip=None, weight_decay=1e-4, loss="mutation", hot=model.hot_parameters(True))
    g = torch.Generator(device="cpu").manual_seed(1234)
    x = torch.randn(16, 1, 512, 512, generator=g).to(dev)
    lab = torch.randint(0, 9, (16, 32, 32), generator=g).to(dev)
    lab = torch.nn.functional.interpolate(lab[:, None].float(), size=(512, 512), mode="nearest")[:, 0].long()
    m = (lab, torch.stack([(lab != k).float() for k in range(9)], 1))
    tr.capture(x, m, warmup=2)
    el = _timed_replay(tr, steps)
    out["emcad_k9_bs16_512"] = {"workload": "EMCADNet dual K=9 (pvt_v2_b2 + EMCAD decoder) fwd + 15-subset CE/Dice/BCE loss + bwd + AdamW, bs=16 512x512 bf16 (config 5, one GPU)",
                                "value": round(16 / el, 1), "unit": "images/sec", "ms_per_step": round(1e3 * el, 3), "steps": steps}
    try:
        out["emcad_k9_bs16_512"]["roofline"] = _config_roofline(tr, x, m)
    except Exception as e:          # noqa: BLE001
        out["emcad_k9_bs16_512"]["roofline"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    del tr, model
    torch.cuda.empty_cache()
    return out


def torch_structure_loss(pred, pred_bg, mask_fg, mask_bg):
    """What an UNEDITED MyTrain_med.py runs (its own structure_loss, :19-38): plain torch ops on the GPU, the 31 x 31 average pool recomputed in each of the four
    calls.  Restated from the formula (as oracle/pranet_oracle.py does), not imported: the reference cannot travel to the GPU box."""
    import torch.nn.functional as F
    weit = 1 + 5 * torch.abs(F.avg_pool2d(mask_fg, kernel_size=31, stride=1, padding=15) - mask_fg)
    wsum = weit.sum(dim=(2, 3))
    wbce = (weit * F.binary_cross_entropy_with_logits(pred, mask_fg, reduction="none")).sum(dim=(2, 3)) / wsum
    wbce_bg = (weit * F.binary_cross_entropy_with_logits(pred_bg, mask_bg, reduction="none")).sum(dim=(2, 3)) / wsum
    p = torch.sigmoid(pred)
    inter = ((p * mask_fg) * weit).sum(dim=(2, 3))
    union = ((p + mask_fg) * weit).sum(dim=(2, 3))
    wiou = 1 - (inter + 1) / (union - inter + 1)
    return (wbce + wiou + 0.8 * wbce_bg).mean()


def module_surface(dev, x, m, steps=20, verbatim=False):
    """The drop-in path: the loop of MyTrain_med.py:59-86 on the mirror classes - model(images) -> 4 x structure_loss -> loss.backward() -> clip_gradient ->
    torch.optim.Adam.step(); torch autograd around one engine pass, which the call site replays from two hipGraphs (forward, backward) after its first calls.
    verbatim=True: the loss is the script's OWN torch-op structure_loss (torch_structure_loss above) - what an unedited MyTrain_med.py executes;
    verbatim=False: the one edit a user can make, `from pn2.loss import structure_loss` (the fused loss kernels, same signature)."""
    import pn2
    from lib.pranet import PraNet_V2
    from utils.utils import clip_gradient
    if verbatim:
        structure_loss = torch_structure_loss
    else:
        from pn2.loss import structure_loss
    pn2.set_compute_dtype("bf16")
    torch.manual_seed(0)
    model = PraNet_V2(num_class=1).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), 1e-4)
    bg = 1 - m

    def step():
        opt.zero_grad()
        o = model(x)
        loss = structure_loss(o[3], o[7], m, bg) + structure_loss(o[2], o[6], m, bg) + structure_loss(o[1], o[5], m, bg) + structure_loss(o[0], o[4], m, bg)
        loss.backward()
        clip_gradient(opt, 0.5)
        opt.step()
        return loss
    for _ in range(6):           # 2 plain calls, 2 on the call site's arena, the capture, one replay (pn2/graph.py)
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / steps
    fused_opt = bool(getattr(opt, "_pn2_fused", None))
    del model, opt
    torch.cuda.empty_cache()
    what = ("nn.Module surface + torch autograd + utils.clip_gradient + torch.optim.Adam, loop of MyTrain_med.py:59-86 with the script's OWN torch-op structure_loss (:19-38, "
            "4 calls, 31x31 avg_pool2d each) - what an unedited script runs" if verbatim else
            "the same loop with ONE edit: structure_loss imported from pn2.loss (fused loss kernels) instead of the script's torch-op version")
    return {"what": what + "; the model call replays two hipGraphs" + ("; clip_gradient + Adam.step run as one clamp launch + pn2_clamp_adam over the flat arenas" if fused_opt else "; clip / Adam are eager torch"),
            "loss_impl": "torch ops (script verbatim)" if verbatim else "pn2.loss.structure_loss (swapped in)", "value": round(x.shape[0] / el, 1),
            "unit": "images/sec", "ms_per_step": round(1e3 * el, 3), "steps": steps, "loss": round(float(loss), 4)}


def inference(dev, reps=50):
    """BASELINE config 1 on the GPU: eval-mode forward of one 352x352 image (MyTest_med.py:98-104) replayed from a hipGraph (pn2.infer.Predictor; conv + BatchNorm
    + ReLU + residual in one launch per layer), and at bs=16 (the largest batch of the published FPS table, jittor/README.md:109-117)."""
    import pn2
    from pn2.infer import Predictor
    from lib.pranet import PraNet_V2
    pn2.set_compute_dtype("bf16")
    torch.manual_seed(0)
    model = PraNet_V2(num_class=1).to(dev).eval()
    out = {}
    with torch.no_grad():
        pred = Predictor(model)
        for bs in (1, 16):
            x = torch.randn(bs, 3, 352, 352, device=dev)
            pred(x); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                pred(x)
            torch.cuda.synchronize()
            el = (time.perf_counter() - t0) / reps
            out[f"bs{bs}_352"] = {"ms_per_batch": round(1e3 * el, 3), "images_per_sec": round(bs / el, 1)}
    del pred, model
    torch.cuda.empty_cache()
    return out


def dp1_line(dev, x, m, steps=10):
    """The data-parallel path on a ONE-rank RCCL communicator (bucket hooks, graph segments, ncclAllReduce between them) next to the local trainer: what the DP
    machinery costs with zero bytes on the wire."""
    import torch.distributed as dist
    import pn2
    from pn2.trainer import Trainer
    from lib.pranet import PraNet_V2
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", str(29400 + os.getpid() % 500))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        pn2.set_compute_dtype("bf16")
        torch.manual_seed(0)
        model = PraNet_V2(num_class=1).to(dev).train()
        tr = Trainer(model, lr=1e-4, clip=0.5, process_group=dist.group.WORLD, force_dp=True)
        tr.capture(x, m, warmup=2)
        el = _timed_replay(tr, steps)
        st_ = tr._cur
        res = {"ms_per_step": round(1e3 * el, 3), "images_per_sec": round(x.shape[0] / el, 1), "graph_segments": len(st_.segments) if st_.segments else 1,
               "collectives": "captured in the step graph" if st_.graph_opt is None else "c10d asynchronous, between graph segments",
               "buckets": len(tr.buckets.buckets), "bucket_mb": [round((e - a) * 4 / 2 ** 20, 1) for a, e, _ in tr.buckets.buckets],
               "allreduce_bytes_per_step": int(tr.n_hot * 4), "backend": "nccl (RCCL), one-rank communicator"}
        del tr, model
    finally:
        dist.destroy_process_group()
    torch.cuda.empty_cache()
    return res


DUMP_SAMPLE = 1 << 21          # elements kept of an output larger than this (8 MB of float32)


def dump_outputs(d, tr, loss):
    """--dump-outputs: what the timed step (Trainer.step / replay) hands its caller after the last timed step, as float32 .npy files in `d`:
      loss.npy    the step's loss vector [loss2, loss3, loss4, loss5, total]
      logits.npy  Trainer.last_outs, the 8 lateral logit maps [8, N, H, W] flattened (res2net / pvt; the mutation loss keeps none)
      weights.npy the trained weights after the optimizer step (the flat fp32 arena every model parameter is a view of)
    An array with more than DUMP_SAMPLE elements is sampled at DUMP_SAMPLE flat indices drawn from a generator seeded per name (sorted, fixed for a
    given shape), so that two builds run with the same arguments can be compared element for element."""
    import numpy as np
    os.makedirs(d, exist_ok=True)

    def put(name, t, seed):
        t = t.detach().reshape(-1)
        if t.numel() > DUMP_SAMPLE:
            g = torch.Generator(device="cpu").manual_seed(seed)
            idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=g).sort().values
            t = t[idx.to(t.device)]
        np.save(os.path.join(d, name + ".npy"), t.float().cpu().numpy())          # (the copy to the host waits for the step)
    put("loss", loss, 0)
    if tr.last_outs is not None:
        put("logits", tr.last_outs, 1)
    put("weights", tr.flat, 2)


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def profiler_attached(env=None):
    """True when a rocprofiler / roctracer tool library rides in this process' environment (rocprofv3 -- python3 bench.py ...).  Its preloaded library has
    initialised the GPU before main() runs, and a process that has done so must not start (or become) a launcher of GPU ranks on this pool: that hop takes the
    machine down.  Profile ONE rank directly (no --gpus N), and put torchrun OUTSIDE the profiler for anything multi-rank."""
    env = os.environ if env is None else env
    if any("rocprof" in env.get(k, "").lower() or "roctracer" in env.get(k, "").lower() for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB")):
        return True
    return any(k.startswith(("ROCPROFILER_", "ROCPROF_", "ROCPROFV3_")) for k in env)


def count_gpus_sysfs(root="/sys/class/kfd/kfd/topology/nodes"):
    """GPUs of this node from the kfd topology (nodes with simd_count > 0) - no HIP / HSA call, so the launcher process never initialises the GPU
    (torch.cuda.device_count() goes through hipGetDeviceCount -> hsa_init when amdsmi is absent).  None when there is a /dev/kfd but no readable topology:
    the ranks themselves then fail on a missing device."""
    try:
        nodes = os.listdir(root)
    except OSError:
        return None if os.path.exists("/dev/kfd") else 0          # no kfd driver at all: no GPUs; a device node without a readable topology: unknown
    n = 0
    for d in nodes:
        try:
            with open(os.path.join(root, d, "properties")) as f:
                props = dict(ln.split()[:2] for ln in f if len(ln.split()) >= 2)
            n += 1 if int(props.get("simd_count", "0")) > 0 else 0
        except (OSError, ValueError):
            continue
    vis = os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES"))
    if vis is not None and vis.strip() != "":
        n = min(n, len([v for v in vis.split(",") if v.strip() != ""]))
    return n


def _die_with_parent():
    """preexec of the launcher child: SIGTERM when this process dies (PR_SET_PDEATHSIG) - a harness that SIGKILLs bench.py does not leave torchrun and its N
    GPU ranks behind (torchrun's agent forwards SIGTERM to its workers)."""
    import ctypes, signal
    try:
        ctypes.CDLL(None, use_errno=True).prctl(1, int(signal.SIGTERM), 0, 0, 0)          # PR_SET_PDEATHSIG = 1
    except Exception:          # noqa: BLE001
        pass


def launch_ranks(n, argv, backend="nccl", timeout=1800.0, out=None):
    """`bench.py --gpus N` without a launcher around it: start N ranks (one per GPU) with torch.distributed.run as a CHILD process, pass its stdout through (rank 0's JSON
    line), return its exit status.  The reference's counterpart is the one-line nn.DataParallel wrap (multiclass_seg/EMCAD/trainer.py:75-77): as easy to start.
    Runs BEFORE anything in this process touches the GPU (devices are counted from the kfd topology in sysfs, no HIP call) and never replaces this process: a
    child, not an exec.  Refuses (status 2, nothing started) under a profiler - its preloaded library HAS initialised the GPU in this process - and when the node
    shows fewer than N devices.  A rank that hangs: the whole process group of the child is killed after `timeout` seconds and the status is 124.  SIGTERM / SIGHUP /
    SIGINT to this process kill that group too; if this process is SIGKILLed the child gets SIGTERM (PR_SET_PDEATHSIG) and torchrun takes its workers down."""
    import signal, subprocess, threading
    out = sys.stdout if out is None else out
    if profiler_attached():
        print("bench.py: refusing to launch ranks from a profiled process (rocprofiler's preloaded library has already initialised the GPU here, and starting GPU "
              "ranks from such a process takes this pool's machines down).  Profile one rank directly - `rocprofv3 ... -- python3 bench.py` without --gpus - and "
              "run multi-rank jobs with the launcher OUTSIDE the profiler.", file=sys.stderr, flush=True)
        return 2
    if backend == "nccl":
        have = count_gpus_sysfs()
        if have is not None and have < n:
            print(f"bench.py: --gpus {n} needs {n} GPUs, this node shows {have} (kfd topology); nothing was started", file=sys.stderr, flush=True)
            return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + list(argv)
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True, start_new_session=True, preexec_fn=_die_with_parent)

    def kill_group():
        try:
            os.killpg(child.pid, signal.SIGKILL)          # the exact group this function started (start_new_session), never a pattern
        except ProcessLookupError:
            pass

    def on_signal(signum, frame):
        kill_group()
        raise SystemExit(128 + signum)
    old = {}
    if threading.current_thread() is threading.main_thread():
        for sg in (signal.SIGTERM, signal.SIGHUP):
            old[sg] = signal.signal(sg, on_signal)

    def pump():
        for line in child.stdout:
            out.write(line); out.flush()
    t = threading.Thread(target=pump, daemon=True)
    t.start()
    try:
        rc = child.wait(timeout=timeout)
    except subprocess.TimeoutExpired:
        print(f"bench.py: the {n}-rank run did not finish within {timeout:.0f} s; killing its process group", file=sys.stderr, flush=True)
        kill_group()
        child.wait()
        rc = 124
    except KeyboardInterrupt:
        kill_group()
        child.wait()
        raise
    finally:
        for sg, h in old.items():
            signal.signal(sg, h)
    t.join(5)
    return rc


def wire_only(args, world, rank, local):
    """--dry-run: everything of an N-rank run except the model - rendezvous, the gradient buckets of pn2/dp.py over an arena of PraNet-V2's gradient size (122 MB; 4 MB on gloo),
    the barrier + max-over-ranks timing protocol, rank 0's JSON line.  With nccl on GPUs this is the exposed-wire bound of the step's all-reduce; with `--backend gloo` it runs on
    CPUs, which is how tests/test_bench_launcher_cpu.py drives the launcher without a GPU.  `value` is null: no images were processed."""
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "pranet-v2_amd"))
    from pn2.dp import GradBuckets
    if args.backend == "nccl":
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        dist.init_process_group("nccl", device_id=dev)
        n = 30_499_908
    else:
        dev = torch.device("cpu")
        dist.init_process_group(args.backend)
        n = 1 << 20
    g = torch.full((n,), float(rank + 1), dtype=torch.float32, device=dev)
    bk = GradBuckets(g, [(0, 0, n // 8), (1, n // 8, n - n // 8)], process_group=dist.group.WORLD)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()
    def step():
        bk.reduce_all()
    for _ in range(args.warmup):
        step()
    sync(); dist.barrier(); sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync(); dist.barrier(); sync()
    el = time.perf_counter() - t0
    t = torch.tensor([el], device=dev, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    el = float(t)
    g.fill_(float(rank + 1))
    bk.reduce_all(); sync()
    ok = bool((g == world * (world + 1) / 2).all())
    if rank == 0:
        print(json.dumps({"metric": "images/sec (train fwd+bwd) at 352x352 bs=32/GPU", "value": None, "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(1e3 * el / max(args.steps, 1), 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "dry_run": True, "config": {"workload": f"dry run: bucketed gradient all-reduce only ({4 * n / 2 ** 20:.0f} MB fp32 arena, no model)", "parallelism": f"dp{world}"},
                          "dp": {"backend": args.backend + (" (RCCL)" if args.backend == "nccl" else ""), "nccl_ranks": world, "buckets": len(bk.buckets), "allreduce_bytes_per_step": 4 * n,
                                 "sum_correct": ok, "bus_GBps": round(2 * (world - 1) / world * 4 * n / (el / max(args.steps, 1)) / 1e9, 2)}}), flush=True)
    dist.destroy_process_group()
    return 0 if ok else 1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=150, help="timed steps (default: ~2 s of hipGraph replay)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU")
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp32fast"])
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--model", default="res2net", choices=["res2net", "pvt", "emcad"],
                    help="res2net = BASELINE config 2/3 (headline); pvt = config 4 (PVT_PraNet_V2, use --batch 16); "
                         "emcad = config 5 (EMCADNet dual K=9 + the 15-subset loss + AdamW, use --batch 16 --size 512)")
    ap.add_argument("--dp1", action="store_true", help="single GPU, but through the data-parallel path on a ONE-rank RCCL communicator (bucket hooks, graph "
                                                       "segments, ncclAllReduce between them): validates the RCCL plumbing where only one GPU is available")
    ap.add_argument("--full", action="store_true", help="after the headline, also measure everything else: the instrumented roofline / per-kernel step, the exposed "
                                                        "all-reduce time, the fp32 lines, configs 4 / 5, module surface, inference, one-rank DP, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-fp32-line", action="store_true", help="--full without the fp32 / fp32fast lines")
    ap.add_argument("--no-extras", action="store_true", help="--full without the extra records of the single-GPU run (configs 4 / 5, module surface, inference, one-rank DP)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend of a multi-rank run (nccl = RCCL; gloo only with --dry-run)")
    ap.add_argument("--dry-run", action="store_true", help="launcher + rendezvous + bucketed gradient all-reduce + the timing protocol, no model (see wire_only)")
    ap.add_argument("--launch-timeout", type=float, default=1800.0, help="seconds after which a self-launched multi-rank run is killed (status 124)")
    argv = sys.argv[1:] if argv is None else list(argv)
    args = ap.parse_args(argv)
    if args.backend != "nccl" and not args.dry_run:
        ap.error("--backend gloo is only meaningful with --dry-run (the step itself has no CPU path)")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: become the launcher (before any GPU call; the ranks are children, this process never initialises the GPU)
        return launch_ranks(args.gpus, argv, backend=args.backend, timeout=args.launch_timeout)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" in os.environ and args.gpus != world and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} ranks; reporting n_gpus = {world}", file=sys.stderr, flush=True)
    if args.dry_run:
        return wire_only(args, world, rank, local)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    use_dist = world > 1 or args.dp1
    if use_dist:
        import torch.distributed as dist
        if world == 1:          # --dp1 without torchrun: a one-rank rendezvous on the loopback
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", str(29400 + os.getpid() % 500))
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        else:
            dist.init_process_group("nccl", device_id=dev)
        pg = dist.group.WORLD

    import pn2
    from pn2.trainer import Trainer
    from lib.pranet import PraNet_V2, PVT_PraNet_V2
    pn2.set_compute_dtype(args.dtype)
    torch.manual_seed(0)
    if args.model == "emcad":
        # EMCAD/trainer.py: 1-channel Synapse slices, 9 classes, AdamW(lr 1e-4, wd 1e-4), supervision='mutation' on the dual heads
        from lib.networks import EMCADNet
        model = EMCADNet(num_classes=9, kernel_sizes=[1, 3, 5], expansion_factor=2, activation="relu6", encoder="pvt_v2_b2", pretrain=False, dual=True).to(dev).train()
        tr = Trainer(model, lr=1e-4, clip=None, weight_decay=1e-4, loss="mutation", hot=model.hot_parameters(True), process_group=pg, force_dp=args.dp1)
        g = torch.Generator(device="cpu").manual_seed(1234 + rank)
        x = torch.randn(args.batch, 1, args.size, args.size, generator=g).to(dev)
        lab = torch.randint(0, 9, (args.batch, args.size // 16, args.size // 16), generator=g).to(dev)
        lab = torch.nn.functional.interpolate(lab[:, None].float(), size=(args.size, args.size), mode="nearest")[:, 0].long()
        m = (lab, torch.stack([(lab != k).float() for k in range(9)], 1))
    else:
        model = (PraNet_V2 if args.model == "res2net" else PVT_PraNet_V2)(num_class=1).to(dev).train()
        tr = Trainer(model, lr=1e-4, clip=0.5, process_group=pg, force_dp=args.dp1)
        x, m = synthetic(args.batch, args.size, 1234 + rank, dev)

    use_graph = not args.no_graph
    if use_graph:
        tr.capture(x, m, warmup=2)
        step = lambda: tr.replay()
    else:
        step = lambda: tr.step(x, m)
    for _ in range(args.warmup):
        loss = step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t)
    loss_v = [float(v) for v in loss.float().cpu()]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tr, loss)

    roof = None
    if args.full:
        # ---- instrumented extra step: per-kernel-family HIP-event timing (not part of the timed region)
        from pn2 import profile as prof
        roof = prof.measure_step(tr, x, m, args.dtype, config={"model": args.model, "batch": args.batch, "size": args.size, "dtype": args.dtype})
    # ---- data-parallel exchange: how much of the gradient all-reduce is exposed (time of a step with the collectives minus one without; --full)
    dp = None
    if use_dist:
        def timed(fn, n=5):
            torch.cuda.synchronize(); dist.barrier(); t0_ = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0_) / n
        st_ = tr._cur
        t_all = timed(step) if args.full else None
        def no_exchange():          # the same graphs without the collectives
            for g_ in ([g for g, _ in st_.segments] if st_.segments else [st_.graph]):
                g_.replay()
            st_.graph_opt.replay()
        t_noex = None
        if args.full and use_graph and st_.graph_opt is not None:
            # the probe steps the optimizer on UNREDUCED local gradients: replicas would silently diverge - restore weights and Adam state after it
            keep = [t_.clone() for t_ in (tr.flat, tr.exp_avg, tr.exp_avg_sq, tr.bias_corr)]
            t_noex = timed(no_exchange)
            for d_, s_ in zip((tr.flat, tr.exp_avg, tr.exp_avg_sq, tr.bias_corr), keep):
                d_.copy_(s_)
            del keep
        dp = {"backend": "nccl (RCCL)", "nccl_ranks": world, "buckets": len(tr.buckets.buckets), "bucket_mb": [round((e - a) * 4 / 2 ** 20, 1) for a, e, _ in tr.buckets.buckets], "allreduce_bytes_per_step": int(tr.n_hot * 4),
              "graph_segments": len(st_.segments) if st_.segments else 1, "wire_dtype": os.environ.get("PN2_DP_WIRE", "fp32"),
              "collectives": ("captured in the step graph" if (use_graph and st_.graph_opt is None) else "c10d asynchronous, between graph segments") if use_graph else "eager",
              "mode": "one-rank communicator on one GPU (--dp1)" if args.dp1 and world == 1 else "one process per GPU",
              "exposed_comm_ms": None if t_noex is None else round(1e3 * (t_all - t_noex), 3)}
    names = {"res2net": "PraNet-V2 Res2Net50", "pvt": "PVT-PraNet-V2 (pvt_v2_b2, DropPath 0.1)", "emcad": "EMCADNet dual K=9 (pvt_v2_b2 encoder, EMCAD decoder)"}
    what = ("fwd+15-subset CE/Dice/BCE loss+bwd+AdamW" if args.model == "emcad" else "fwd+4x structure_loss+bwd+clamp+Adam")

    if rank == 0:
        ips = world * args.batch * args.steps / el
        out = {
            "metric": "images/sec (train fwd+bwd) at 352x352 bs=32/GPU",
            "value": round(ips, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * el / args.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{names[args.model]} training step ({what}), bs={args.batch}/GPU {args.size}x{args.size}, "
                                   f"random-init, synthetic {'block labels' if args.model == 'emcad' else 'ellipse masks'}", "global_batch": world * args.batch, "parallelism": f"dp{world}",
                       "launch": "hipGraph replay" if use_graph else "eager"},
            "loss": loss_v,
            "mfma_frac_whole_step": (None if args.model == "emcad" else
                                     round(ips / world * (TRAIN_GFLOP_PER_IMG if args.model == "res2net" else 72.3) / 1e3 / (PEAK_BF16_TFLOPS if args.dtype == "bf16" else PEAK_F32_TFLOPS), 4)),
        }
        if roof is not None:
            out["roofline"], out["kernels"] = roof["roofline"], roof["kernels"]
            hb = out["roofline"].get("step_hbm_bytes_pmc")
            if hb:          # the whole step against the HBM roofline: bytes of the committed PMC passes / this run's step time (the step is traffic-bound first)
                gbs = hb / (1e-3 * out["ms_per_step"]) / 1e9
                out["roofline"]["step_hbm"] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(gbs / 8000.0, 4), "bytes_per_step": hb,
                                              "source": out["roofline"].get("traffic_source"), "source_commit": out["roofline"].get("traffic_commit"),
                                              "note": "bytes: PMC passes (FETCH_SIZE x 2 + WRITE_SIZE, eager launches) recorded at source_commit - a derived figure, stale "
                                                      "if kernels that move data changed after that commit; time: this run"}
        # always present: how many ranks exchanged gradients (1 = a single process, no collective on the data path)
        out["dp"] = dp if dp is not None else {"backend": None, "nccl_ranks": 1, "mode": "single process, no collective on the data path"}
        if args.full and world == 1 and not args.no_fp32_line and args.model == "res2net" and args.dtype == "bf16":
            tr = None
            torch.cuda.empty_cache()
            out["fp32"] = fp32_line(lambda: PraNet_V2(num_class=1).to(dev).train(), x, m)
            torch.cuda.empty_cache()
            out["fp32fast"] = fp32_line(lambda: PraNet_V2(num_class=1).to(dev).train(), x, m, mode="fp32fast")
        if args.full and world == 1 and not args.no_extras and not args.dp1 and args.model == "res2net" and args.dtype == "bf16" and args.batch == 32 and args.size == 352:
            # the other numbers of the repository, in the driver's record (each bounded to a few seconds of GPU time; a failure is reported, not fatal)
            tr = None
            torch.cuda.empty_cache()
            for key, fn in (("configs", lambda: other_configs(dev)), ("module_surface_verbatim", lambda: module_surface(dev, x, m, verbatim=True)),
                            ("module_surface", lambda: module_surface(dev, x, m)), ("inference", lambda: inference(dev)),
                            ("dp1", lambda: dp1_line(dev, x, m))):
                try:
                    out[key] = fn()
                except Exception as e:          # noqa: BLE001
                    out[key] = {"error": f"{type(e).__name__}: {e}"[:300]}
            if "dp1" in out and "ms_per_step" in out["dp1"]:
                out["dp1"]["local_ms_per_step"] = out["ms_per_step"]
                out["dp1"]["overhead_frac"] = round(out["dp1"]["ms_per_step"] / out["ms_per_step"] - 1.0, 4)
        if args.full and world == 1 and not args.no_cpu_baseline and args.model != "emcad":
            out["cpu_baseline"] = cpu_baseline(args.size)
        try:          # libraries that printf to the C stdout of a pipe (RCCL's version banner) are flushed first: the JSON line stays the last line of stdout
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
