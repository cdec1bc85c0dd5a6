"""DPM-Solver++(2M) beside DDIM on one GPU, two measurements:
  kernel      c2d_cfg_dpm_step and c2d_cfg_ddim_step at the c3 shape (B = 8, 64 x 64 latents): 200 launches of
              the step (without the counter advance, so every launch does a middle step's work) captured in one
              graph and replayed, the two kernels alternated;
  end to end  images/s of generate_batch_graphed at --batch / --res for each "sampler:steps" of --configs
              (default 50-step DDIM and 20-step dpmpp_2m), warmed up, then timed alternately --reps times.
A step costs the same whatever the solver (the UNet dominates), so the throughput ratio is the step ratio; this
script measures it.  It says nothing about image quality: the weights are the seeded synthetic recipe."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from clap2diffusion_amd import ops  # noqa: E402
from clap2diffusion_amd.pipeline import AudioToImageInference, initial_latents, synthetic_thunder  # noqa: E402
from clap2diffusion_amd.scheduler import DPMSolverMultistepScheduler  # noqa: E402
from clap2diffusion_amd.text_encoder import tokenize  # noqa: E402

LAUNCHES, REPLAYS, ROUNDS = 200, 10, 5


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    return g


def replay_us(g) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * LAUNCHES)


def kernel_times(dev, b: int = 8, hw: int = 64, steps: int = 20) -> None:
    sched = DPMSolverMultistepScheduler()
    sched.set_timesteps(steps)
    _, coef, mcoef = sched.device_tables(dev)
    eps = torch.randn(2 * b, hw, hw, 4, device=dev).half()
    x, x0_prev = torch.randn(b, 4, hw, hw, device=dev), torch.randn(b, 4, hw, hw, device=dev)
    idx = torch.full((1,), steps // 2, dtype=torch.int32, device=dev)
    first = torch.zeros(1, dtype=torch.int32, device=dev)
    graphs = {"c2d_cfg_ddim_step": graph_of(lambda: ops.cfg_ddim_step(eps, x, 1.0, coef, idx, advance=False)),
              "c2d_cfg_dpm_step": graph_of(lambda: ops.cfg_dpm_step(eps, x, x0_prev, 1.0, mcoef, idx, first,
                                                                    advance=False))}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):
        for name, g in graphs.items():
            times[name].append(replay_us(g))
    for name, t in times.items():
        print(f"kernel {name} B={b} {hw}x{hw}: median {statistics.median(t):.2f} us per graph-replayed launch "
              f"(min {min(t):.2f}, max {max(t):.2f}, {ROUNDS} rounds of {REPLAYS} x {LAUNCHES})", flush=True)


def throughput(dev, batch: int, res: int, configs: list, reps: int) -> None:
    pipe = AudioToImageInference(device=dev, height=res, width=res, verbose=False)
    clips = pipe.feature_extractor.crop([synthetic_thunder(i) for i in range(batch)])
    wave = torch.from_numpy(np.concatenate(clips)).to(dev)
    lens = torch.tensor([c.size for c in clips], dtype=torch.int32, device=dev)
    offs = torch.tensor(np.cumsum([0] + [c.size for c in clips[:-1]]), dtype=torch.int64, device=dev)
    ids = (tokenize([""] * batch, dev), tokenize(["a thunderstorm over the sea"] * batch, dev))
    lat = initial_latents(list(range(batch)), res // 8, res // 8, dev)

    def one(sampler, steps):
        return pipe.generate_batch_graphed(wave, offs, lens, ids, lat, steps, 7.5, sampler=sampler)
    for sampler, steps in configs:                              # capture, then one replayed run
        for _ in range(2):
            one(sampler, steps)
    torch.cuda.synchronize()
    rates = {c: [] for c in configs}
    for _ in range(reps):
        for c in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            img = one(*c)
            e1.record()
            e1.synchronize()
            assert torch.isfinite(pipe.last_denoiser.x).all() and img.shape[0] == batch
            rates[c].append(batch / (e0.elapsed_time(e1) * 1e-3))
    for (sampler, steps), r in rates.items():
        print(f"end to end {sampler} {steps} steps B={batch} {res}x{res}: median {statistics.median(r):.3f} images/s "
              f"(min {min(r):.3f}, max {max(r):.3f}, {reps} runs)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", nargs="+", default=["ddim:50", "dpmpp_2m:20"], metavar="SAMPLER:STEPS")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true")
    a = ap.parse_args()
    configs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.configs]
    dev = torch.device("cuda")   # no GPU: this raises, there is no fallback
    if not a.no_kernel:
        kernel_times(dev)
    if not a.no_end_to_end:
        with torch.no_grad():
            throughput(dev, a.batch, a.res, configs, a.reps)


if __name__ == "__main__":
    main()
