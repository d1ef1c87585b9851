"""GPU: rala with RALA_DEVICE_CONTIGS=1 - the nodes of the assembly graph as spans of a table of bases on the device, contigs,
unitigs and -p reads spelled there - prints byte for byte what it prints without the switch, and says that it took that path."""
import gzip
import os
import re
import subprocess

import pytest

from rala_amd import build
from rala_amd.synth import Dataset

import test_sequences_cpu as host

pytestmark = pytest.mark.gpu

COUNTS = ("transitive edges", "tips", "bubbles", "long edges")


def _files(tmp_path, n, genome, seed):
    ds = Dataset(n, genome, seed)
    fa, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "ovl.paf")
    ds.write_fasta(fa)
    ds.write_paf(paf)
    return ds, fa, paf


def _run(args, env=None, **switches):
    exe = os.path.join(build.PKG, "host", "rala")
    env = dict(os.environ if env is None else env, **switches)
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def _counts(err):
    return [int(re.search(r"number of %s = (\d+)" % what, err).group(1)) for what in COUNTS]


def _took_the_device_path(err, spelled=True):
    assert re.search(r"\[rala::Graph::construct\] node bases on the device: \d+ sources, \d+ bytes", err), err[-2000:]
    assert "node bases on the host" not in err
    if spelled:
        assert re.search(r"\[rala::Graph::extract_contigs\] spelled \d+ bytes on the device", err), err[-2000:]


@pytest.mark.parametrize("n,genome,seed", [(600, 120_000, 17), (3000, 400_000, 5), (2000, 1_000_000, 3)])
def test_unitigs_and_debug_files_equal_the_string_path(tmp_path, n, genome, seed):
    build.build_host()
    _, fa, paf = _files(tmp_path, n, genome, seed)
    off = _run(["-u", "-d", str(tmp_path / "off"), fa, paf])
    on = _run(["-u", "-d", str(tmp_path / "on"), fa, paf], RALA_DEVICE_CONTIGS="1")
    _took_the_device_path(on[1])
    assert "on the device" not in off[1]
    assert on[0] == off[0] and off[0].count(b">Ctg") > 0 and len(off[0]) > genome // 2
    for ext in (".csv", ".json"):
        assert open(str(tmp_path / "on") + ext, "rb").read() == open(str(tmp_path / "off") + ext, "rb").read()
    assert _counts(on[1]) == _counts(off[1])
    spelled = int(re.search(r"spelled (\d+) bytes on the device", on[1]).group(1))
    assert spelled == sum(len(l) for l in off[0].split(b"\n") if l and not l.startswith(b">"))


def test_contigs_and_preconstruct_reads_equal_the_string_path(tmp_path):
    build.build_host()
    _, fa, paf = _files(tmp_path, 3000, 400_000, 5)
    off, on = _run([fa, paf]), _run([fa, paf], RALA_DEVICE_CONTIGS="1")
    _took_the_device_path(on[1])
    assert on[0] == off[0] and off[0].count(b">Ctg") > 0
    off, on = _run(["-p", fa, paf]), _run(["-p", fa, paf], RALA_DEVICE_CONTIGS="1")
    _took_the_device_path(on[1], spelled=False)
    assert on[0] == off[0] and off[0].count(b">") > 100


def test_gzip_fastq_the_table_is_what_the_slice_kept(tmp_path):
    """the read file one gzip member, indexed and sliced on the device: the bases never reach the host before the contigs do"""
    build.build_host()
    ds, fa, paf = _files(tmp_path, 3000, 400_000, 5)
    lines = open(fa, "rb").read().split(b"\n")
    pairs = [(lines[2 * i][1:], lines[2 * i + 1]) for i in range(ds.n_reads)]
    fq = str(tmp_path / "reads.fastq.gz")
    open(fq, "wb").write(gzip.compress(host.fastq_text(pairs), 6))
    off = _run(["-u", fq, paf])
    on = _run(["-u", fq, paf], RALA_DEVICE_SEQUENCES="1", RALA_DEVICE_GZIP="1", RALA_DEVICE_CONTIGS="1")
    _took_the_device_path(on[1])
    line = [l for l in on[1].split("\n") if "node bases on the device" in l][0]
    assert "kept by the device's slice" in line             # (rala_hip_get_spell_info's from_slice)
    assert on[0] == off[0] and len(off[0]) > 200_000
    # without the device's index the bases come from the host reader and are handed over: the same bytes
    handed = _run(["-u", fq, paf], RALA_DEVICE_CONTIGS="1")
    _took_the_device_path(handed[1])
    assert "kept by the device's slice" not in handed[1] and handed[0] == off[0]


def test_two_ranks(tmp_path):
    """rala --gpus 2, the ranks on device 0 over the in-process transport: the table lives on the graph's context"""
    build.build_host()
    _, fa, paf = _files(tmp_path, 3000, 400_000, 5)
    many = dict(os.environ, RALA_COMM="local", RALA_GPU_DEVICES="0,0")
    off = _run(["-u", "--gpus", "2", fa, paf], env=many)
    on = _run(["-u", "--gpus", "2", fa, paf], env=many, RALA_DEVICE_CONTIGS="1")
    _took_the_device_path(on[1])
    one = _run(["-u", fa, paf])
    assert on[0] == off[0] == one[0] and one[0].count(b">Ctg") > 0
