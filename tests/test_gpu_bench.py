"""-m gpu: the bench.py contract executed -- the one JSON line at N = 1 (a plain run: the headline alone; --full: headline, roofline
with every byte model, the attached 16-bit legs and the configs[4] share) and the N = 2 launch the driver uses (torch.distributed.run, here two ranks
sharing the one GPU with gloo standing in for RCCL)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


LINE_LIMIT = 3800   # bytes: round 5's 27 KB line came back from the driver as `parsed: null`


def _line(stdout):
    rows = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 1, stdout[-3000:]      # exactly ONE stdout line opens a JSON object
    assert len(rows[0].encode()) <= LINE_LIMIT, len(rows[0])
    return json.loads(rows[0])


def _check_leg_roofline(roof):
    assert roof["bound"] in ("mfma", "hbm") and roof["unit"] == ("TFLOP/s" if roof["bound"] == "mfma" else "GB/s")
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-4 and 0 < roof["frac"] < 1.0 and roof["avg_launch_us"] > 0
    assert "kernels" not in roof and "fractions_legend" not in roof


def _check_roofline(roof, dtype):
    assert roof["bound"] in ("mfma", "hbm") and roof["unit"] == ("TFLOP/s" if roof["bound"] == "mfma" else "GB/s")
    fr = roof["fractions"]
    assert set(fr) == {"frac_mfma", "frac_hbm_min", "frac_hbm_m1", "frac_hbm_pmc"}
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9 and roof["frac"] == fr[roof["frac_is"]]
    hbm = fr["frac_hbm_pmc"] if fr["frac_hbm_pmc"] is not None else fr["frac_hbm_min"]
    assert roof["frac"] == max(fr["frac_mfma"], hbm)
    for k in roof["kernels"]:
        assert k["bytes_min"] > 0 and k["bytes_m1"] >= 0 and 0 < k["frac_mfma"] < 1.0 and 0 < k["frac_hbm_min"] < 1.0
    dom = roof["kernels"][0]
    assert dom["kernel"] == roof["kernel"] and dom["bytes_m1"] > dom["bytes_min"]   # a fused kernel: M1 charges more than the launch can move


def test_plain_line_is_the_headline_alone(native_lib, cuda, tmp_path):
    """Without --full the run sets up, warms up, times its steps, dumps and prints the line: no roofline pass, no legs, no cpu_baseline,
    no side file."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames-per-step", "32", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = _line(r.stdout)
    assert {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "warmup_settle", "dumped_outputs"} == set(d)
    assert d["metric"] == "frames/sec (7-view 2D->3D)" and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and "configs[1]" in d["config"]["workload"]
    assert abs(d["value"] - 64 / (2 * d["ms_per_step"] * 1e-3)) < 1e-5 * d["value"]
    assert d["dumped_outputs"] == {"points2d": [7, 32, 38, 2], "heatmap_confidence": [7, 32, 19], "points3d": [32, 38, 3]}
    assert sorted(os.listdir(out)) == ["heatmap_confidence.npy", "points2d.npy", "points3d.npy"]


def test_full_line_has_every_leg_and_every_fraction(native_lib, cuda):
    r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--frames-per-step", "32", "--cpu-seconds", "2", "--full"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    short = _line(r.stdout)
    # the short line: headline + roofline (no tables) + legs + cpu_baseline, and the side file it names holds the whole record
    assert {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline", "cpu_baseline", "config1_f32_split", "config2_bf16", "config2_f16", "config4_share"} <= set(short)
    assert {"bound", "kernel", "achieved", "peak", "unit", "frac", "traffic"} <= set(short["roofline"]) and "kernels" not in short["roofline"]
    assert abs(short["roofline"]["frac"] - short["roofline"]["achieved"] / short["roofline"]["peak"]) < 1e-4
    for key, kern in (("config1_f32_split", "F32S"), ("config2_bf16", "__hip_bfloat16"), ("config2_f16", "_Float16")):
        _check_leg_roofline(short[key]["roofline"])
        assert kern in short[key]["roofline"]["kernel"], short[key]["roofline"]   # the leg ran its own engine's kernels, not a fallback
    assert "bottleneck_wino_f32_kernel" in short["roofline"]["kernel"]   # the exact-fp32 engine's default tail (round 6: Winograd)
    # roofline honesty: the fraction is EXECUTED FLOPs over the peak (< 1); the direct-convolution rate of the same launches is printed beside it
    assert short["roofline"]["frac"] < 1.0 and short["roofline"]["direct_equivalent_tflops"] > short["roofline"]["achieved"]
    with open(os.path.join(ROOT, short["tables"])) as f:
        d = json.load(f)
    assert abs(d["value"] - short["value"]) < 1e-4 * d["value"]
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["dtype"] == "f32" and d["unit"] == "frames/s" and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert abs(d["value"] - 64 / (2 * d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert "configs[1]" in d["config"]["workload"]
    # BASELINE's second metric (hourglass HBM GB/s vs peak) by three byte models: least possible <= counted (when traffic.json covers the step) <= M1
    c = d["config"]
    assert 0 < c["hourglass_gbs_min_end_to_end"] < c["hourglass_gbs_m1_end_to_end"] and c["hourglass_frac_hbm_m1_end_to_end"] < 1.0
    if "hourglass_gbs_pmc_end_to_end" in c:
        assert 0.9 * c["hourglass_gbs_min_end_to_end"] < c["hourglass_gbs_pmc_end_to_end"] < 8000.0
    _check_roofline(d["roofline"], "f32")
    assert d["roofline"]["bound"] == "mfma" and "bottleneck_wino_f32_kernel" in d["roofline"]["kernel"]
    assert 0 < c["hourglass_frac_mfma_end_to_end"] < 1.0 and c["hourglass_tflops_executed_end_to_end"] < c["hourglass_tflops_end_to_end"]
    for key, dt in (("config1_f32_split", "f32s"), ("config2_bf16", "bf16"), ("config2_f16", "f16")):
        leg = d[key]
        assert leg["dtype"] == dt and leg["value"] > 0 and ("configs[1]" if dt == "f32s" else "configs[2]") in leg["workload"]
        assert abs(leg["value"] - 64 / (leg["steps"] * leg["ms_per_step"] * 1e-3)) < 1e-6 * leg["value"]
        _check_roofline(leg["roofline"], dt)
    # the split-product leg carries its price: its heat-maps against the exact-fp32 engine's, inside the fp32 test tolerance, same cells
    assert d["config1_f32_split"]["max_rel_diff_vs_f32_engine"] < 5e-5
    sh = d["config4_share"]
    assert "error" not in sh, sh
    assert sh["frames"] == 2000 and sh["bundle_adjust_runs"] == 2 and sh["gather_roundtrip_exact"] is True and sh["collective_backend"] == "nccl"
    assert sh["value"] > 0
    # a loose ORDER of the rates (bench.py settles the clocks before it times; the measured ratios are 1.8x / 3x): a leg that silently ran a slow or
    # fallback path would land below the exact-fp32 engine
    assert d["config1_f32_split"]["value"] > d["value"] and d["config2_bf16"]["value"] > d["value"] and d["config2_f16"]["value"] > d["value"]
    print("rates (frames/s): f32", round(d["value"], 1), "f32 split", round(d["config1_f32_split"]["value"], 1), "bf16", round(d["config2_bf16"]["value"], 1), "f16", round(d["config2_f16"]["value"], 1),
          "configs[4] share", round(sh["value"], 1), "cpu port", round(d["cpu_baseline"]["value"], 3))
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0


def test_two_ranks_over_gloo_share_the_gpu(native_lib, cuda):
    """The driver's N > 1 launch line, on the one GPU at hand: both ranks run their own frame range, the gather executes (gloo),
    rank 0 prints one line with n_gpus 2 and the aggregate rate -- about the 1-rank rate, since the two ranks share the device."""
    env = dict(os.environ, DF3D_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    common = ["--steps", "3", "--warmup", "1", "--frames-per-step", "32", "--dtype", "f16", "--no-cpu-baseline", "--no-roofline", "--verify"]
    one = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-4000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29641",
                          "bench.py", "--gpus", "2"] + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-4000:]
    d1, d2 = _line(one.stdout), _line(two.stdout)
    assert d1["n_gpus"] == 1 and d1["config"]["collective_executed"] is False
    assert d2["n_gpus"] == 2 and d2["config"]["collective_executed"] is True and d2["config"]["collective_backend"] == "gloo"
    assert d2["config"]["frames_per_gpu"] == 96 and "config2_bf16" not in d2
    # --verify: rank 0 regenerated rank 1's seeded frames, ran them through its own pipeline and found rank 1's gathered records bit-identical
    assert d1["verify"] == {"frames_recomputed_on_rank0": 6, "ranks_sampled": 1, "bit_identical": True, "ranks_differing": []}
    assert d2["verify"] == {"frames_recomputed_on_rank0": 12, "ranks_sampled": 2, "bit_identical": True, "ranks_differing": []}
    assert len(d2["per_rank_frames_per_s"]) == 2 and d2["rccl_world"] == 2 and d2["gather_ms"] > 0
    assert abs(d2["value"] - 2 * 96 / (3 * d2["ms_per_step"] * 1e-3)) < 1e-5 * d2["value"]
    # (two ranks on ONE device: the aggregate is about the device's rate; printed, not asserted -- tests/perf/ holds the rate bands)
    print("rates (frames/s): 1 rank", round(d1["value"], 1), "2 ranks on one GPU", round(d2["value"], 1))


def test_strong_scaled_stream_one_rank_and_two_ranks_over_gloo(native_lib, cuda):
    """`--strong`: BASELINE configs[3]/[4] as ONE stream sharded over the ranks, gather + sequence-global Procrustes inside the timed
    region.  N = 1 is the plain single-GPU pipeline plus the Procrustes launch (rates printed; the band lives in tests/perf/); N = 2 (two ranks sharing the
    one GPU, gloo standing in for RCCL) splits the stream by the bundle-adjustment window and reports the stream's rate once."""
    env = dict(os.environ, DF3D_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
    common = ["--warmup", "1", "--frames-per-step", "32", "--dtype", "f16", "--no-cpu-baseline", "--no-roofline"]
    plain = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "12"] + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-4000:]
    one = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--strong", "--stream-frames", "384"] + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-4000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29643",
                          "bench.py", "--gpus", "2", "--strong", "--stream-frames", "360", "--ba-window", "120"] + common, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-4000:]
    d0, d1, d2 = _line(plain.stdout), _line(one.stdout), _line(two.stdout)
    assert d1["scaling"] == "strong" and d1["n_gpus"] == 1 and d1["steps"] == 12 and d1["config"]["frames_per_gpu"] == [384] and "configs[3]" in d1["config"]["workload"]
    assert abs(d1["value"] - 384 / (12 * d1["ms_per_step"] * 1e-3)) < 1e-5 * d1["value"]
    print("rates (frames/s): plain", round(d0["value"], 1), "strong N=1", round(d1["value"], 1), "strong N=2 on one GPU", round(d2["value"], 1))
    assert d2["scaling"] == "strong" and d2["n_gpus"] == 2 and d2["config"]["frames_per_gpu"] == [240, 120] and d2["steps"] == 8   # windows 2 + 1
    assert "configs[4]" in d2["config"]["workload"] and d2["config"]["collective_executed"] is True and d2["config"]["bundle_adjust_runs_rank0"] == 2
    assert abs(d2["value"] - 360 / (8 * d2["ms_per_step"] * 1e-3)) < 1e-5 * d2["value"]
    assert set(d2["config"]["rank0_tail_ms"]) == {"steps_enqueued", "recalibrations_joined", "gather", "procrustes_and_drain"}
