"""The rules of candidate selection's host code, without a GPU: tools/probes/select_rules_probe.hip calls the functions
of alphadia_amd/csrc/adh_select_rules.h that the selection drivers call (rank-1 factors of a smoothing kernel, the
two-row tap table, the refusal of cycles with more than 16 rows per group, the scratch budget, the cutting of batches);
here it is compiled for the host with the address and undefined-behaviour sanitizers and run as a program of its own."""

import os
import subprocess

import __graft_entry__ as entry


def test_select_rules_probe_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "select_rules_probe")
    src = os.path.join(entry.ROOT, "tools", "probes", "select_rules_probe.hip")
    subprocess.run([entry._hipcc(), "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src],
                   check=True, cwd=entry.ROOT)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all selection rules hold" in run.stdout
    assert "runtime error" not in run.stderr
