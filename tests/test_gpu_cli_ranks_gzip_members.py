"""GPU: rala --gpus 2 (ranks as threads over the local transport, both on device 0) from a `cat` of three .paf.gz parts and a -s
file by gzip -6.  With RALA_DEVICE_COMPRESSED=2 RALA_DEVICE_GZIP=2 both ranks inflate a part of BOTH files on the device - the -s
file through rala_hip_mg_tokenise_sensitive, its shares into rala_hip_mg_run - and stdout and the stage lines (the simplify
counts among them) are those of the run without switches, which reads both files on the host; with RALA_DEVICE_COMPRESSED=1
both files stay with the host reader as they did, and RALA_DEVICE_INGEST=0 overrides everything."""
import os
import re
import subprocess

import numpy as np
import pytest

from rala_amd import build
from rala_amd.synth import Dataset

pytestmark = pytest.mark.gpu


def test_cli_over_two_ranks_from_a_cat_of_three_gzip_parts_and_a_gzip_sensitive_file(tmp_path):
    from oracle.oracle import Oracle

    build.build_host()
    exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    fa, paf, sens = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf"), str(tmp_path / "uncontained.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    o = Oracle(ds.read_len, ds.overlaps, n_threads=4)
    assert o.initialize() == 0
    o.pass2()
    o.preprocess_chimeras()
    p = o.piles()
    ds.sensitive(p["alive"], p["begin"], p["end"])
    ds.write_paf(sens, sensitive=True, target_len=(p["end"] - p["begin"]).astype(np.uint32))
    lines = open(paf, "rb").read().splitlines(keepends=True)
    joined = str(tmp_path / "parts.paf.gz")
    with open(joined, "wb") as out:
        for k in range(3):                                      # what `cat part*.paf.gz` gives
            part = str(tmp_path / ("part%d.paf" % k))
            open(part, "wb").write(b"".join(lines[len(lines) * k // 3:len(lines) * (k + 1) // 3]))
            subprocess.run(["gzip", "-6", "-c", part], stdout=out, check=True)
    with open(sens + ".gz", "wb") as out:                       # `minimap2 ... | gzip > uncontained.paf.gz`
        subprocess.run(["gzip", "-6", "-c", sens], stdout=out, check=True)
    two = dict(os.environ, RALA_COMM="local", RALA_GPU_DEVICES="0,0", RALA_HIP_TRACE="1")
    for k in ("RALA_DEVICE_COMPRESSED", "RALA_DEVICE_GZIP", "RALA_DEVICE_INGEST"):
        two.pop(k, None)

    def run(env):
        r = subprocess.run(["timeout", "-k", "10", "300", exe, "-s", sens + ".gz", "--gpus", "2", fa, joined], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env)
        err = r.stderr.decode()
        assert r.returncode == 0, err[-3000:]
        stages = [re.sub(r" \d+\.\d+ s$", "", x) for x in err.splitlines() if x.startswith("[rala::")]
        return r.stdout, stages, err

    off = run(two)
    on = run(dict(two, RALA_DEVICE_COMPRESSED="2", RALA_DEVICE_GZIP="2"))
    assert len(off[0]) > 1000 and any("simplif" in s.lower() for s in off[1]), off[1]
    assert on[:2] == off[:2]
    # both ranks a part of both files: the primary file's three members, the -s file's one
    assert len(re.findall(r"device inflate: part \d of 2 of 3 gzip members", on[2])) == 2, on[2][-3000:]
    assert len(re.findall(r"device inflate: part \d of 2 of 1 gzip members", on[2])) == 2, on[2][-3000:]
    assert "device inflate" not in off[2]
    # RALA_DEVICE_GZIP=1: the -s file of one member over the ranks, the primary file of three members the host reader's
    one = run(dict(two, RALA_DEVICE_COMPRESSED="2", RALA_DEVICE_GZIP="1"))
    assert one[:2] == off[:2]
    assert len(re.findall(r"device inflate: part \d of 2 of one gzip member", one[2])) == 2, one[2][-3000:]
    assert "gzip members" not in one[2]
    for env in (dict(RALA_DEVICE_COMPRESSED="1", RALA_DEVICE_GZIP="2"), dict(RALA_DEVICE_COMPRESSED="2", RALA_DEVICE_GZIP="2", RALA_DEVICE_INGEST="0"),
                dict(RALA_DEVICE_COMPRESSED="2")):
        got = run(dict(two, **env))
        assert got[:2] == off[:2] and "device inflate" not in got[2], env
