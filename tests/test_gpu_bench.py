"""bench.py end to end on one GPU: a plain run with --dump-outputs, and the
N > 1 path: two ranks
started by `bench.py --gpus 2` itself (torch.distributed.run), both on
cuda:0, over gloo (RCCL refuses two ranks on one GPU) -- the launcher,
init_process_group, the checked step, the timed full steps (decode, entry
exchange, any redo), the decode-only steps, the confirmation, the segments'
all-gather and the rank-reduced timing all run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_its_outputs(files_dir, tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W`: the headline line
    without the --full measurements, and --dump-outputs' arrays equal to the
    tiled text (length, both ends, the seeded sample, every block's sum)."""
    import numpy as np
    import bench
    from huffmandecoderongpus_amd import synth
    mib = 16
    res = _run_bench(["--gpus", "1", "--size-mib", str(mib), "--steps", "3", "--warmup", "1",
                      "--dump-outputs", str(tmp_path)])
    assert res["metric"] == "decoded MB/s" and res["unit"] == "MB/s" and res["dtype"] == "u8"
    assert res["higher_is_better"] is True and res["n_gpus"] == 1
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0 and res["value"] > 0
    assert res["fast_path"] is True and res["state_machine_path"] is True
    assert res["roofline"]["ms_kernel"] > 0 and 0 < res["roofline"]["frac"] < 1
    # what --full adds is absent from a plain run
    for k in ("workloads", "evaluate", "encode", "cpu_baseline"):
        assert k not in res
    assert res["ms_per_call_sync"] is None and "copy_GBps" not in res["roofline"]
    assert res["roofline"]["two_pass_split_ms"] == {"count": None, "scan": None, "emit": None}

    hf, text = synth.load_source(files_dir, "kjv.txt")
    _, n = synth.cut_bits(hf, text, mib << 20)
    assert res["config"]["decoded_bytes"] == n
    # value = decoded bytes / time per step (ms_per_step is rounded to 4 places, value to 1)
    ms = res["ms_per_step"]
    assert abs(res["value"] - n / (ms * 1e-3) / 1e6) <= res["value"] * 0.5e-4 / (ms - 0.5e-4) + 0.05
    assert sorted(os.listdir(tmp_path)) == ["decoded_block_sums.npy", "decoded_length.npy", "decoded_symbols.npy"]
    ln, got, sums = (np.load(os.path.join(tmp_path, k + ".npy"))
                     for k in ("decoded_length", "decoded_symbols", "decoded_block_sums"))
    assert ln.dtype == np.float64 and ln.tolist() == [n]
    E, S, B = bench.DUMP_EDGE, bench.DUMP_SAMPLE, bench.DUMP_BLOCK
    assert n > bench.DUMP_WHOLE and got.dtype == np.float32 and got.size == 2 * E + S
    want = np.tile(text, n // text.size + 1)[:n]
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(E, n - E, S))
    assert np.array_equal(got, np.concatenate([want[:E], want[pos], want[n - E:]]).astype(np.float32))
    assert sums.dtype == np.float64
    assert np.array_equal(sums, [want[o:o + B].sum(dtype=np.int64) for o in range(0, n, B)])


def test_bench_two_ranks_gloo_one_device(files_dir):
    from huffmandecoderongpus_amd import synth
    mib = 64
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--size-mib", str(mib), "--steps", "3",
           "--warmup", "1", "--backend", "gloo", "--one-device", "--no-cpu-baseline", "--no-extra"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2
    assert res["settle"]["confirmed_after_timed"] is True
    assert res["allgather"]["seams_ok"] is True
    hf, text = synth.load_source(files_dir, "kjv.txt")
    _, syms = synth.cut_bits(hf, text, 2 * (mib << 20))
    assert res["config"]["decoded_bytes"] == syms
    assert res["value"] > 0 and res["settle"]["decode_only"]["ms_per_step"] > 0
