"""The host side of the compacted copy-out's block formats, without a GPU: tools/probes/sparse_block_probe.hip builds
dense, sparse-slot and fallback blocks by a plain restatement of the formats, expands them with the product's
fill_host_rows (alphadia_amd/csrc/adh_fill_host.h) and compares the tables; here it is compiled for the host with
the address and undefined-behaviour sanitizers and run as a program of its own."""

import os
import subprocess

import __graft_entry__ as entry


def test_sparse_block_probe_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "sparse_block_probe")
    src = os.path.join(entry.ROOT, "tools", "probes", "sparse_block_probe.hip")
    subprocess.run([entry._hipcc(), "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src],
                   check=True, cwd=entry.ROOT)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all blocks expand to the padded tables" in run.stdout
    assert "runtime error" not in run.stderr
