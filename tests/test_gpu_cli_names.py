"""GPU: the command line with the name table built on the device (RALA_DEVICE_NAMES=1 beside RALA_DEVICE_SEQUENCES=1) and
without it: the same contigs, the same stage lines and counts on stderr, the same -d CSV and JSON, on the suite's 20x data set -
for every kind of read file the device indexes, with a duplicated name, with -s, with -p, over two ranks, and where the
tokeniser hands the overlap file back to a host reader, which then probes the table the device built."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from rala_amd import build
from rala_amd.synth import Dataset

import test_sequences_cpu as host

pytestmark = pytest.mark.gpu


class Data:
    pass


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from oracle.oracle import Oracle

    build.build_host()
    d = Data()
    d.dir = tmp_path_factory.mktemp("cli_names")
    d.exe = os.path.join(build.PKG, "host", "rala")
    ds = Dataset(3000, 400_000, 5)
    d.fa, d.paf, d.sens = str(d.dir / "reads.fasta"), str(d.dir / "ovl.paf"), str(d.dir / "sens.paf")
    ds.write_fasta(d.fa)
    ds.write_paf(d.paf)
    lines = open(d.fa, "rb").read().split(b"\n")
    pairs = [(lines[2 * i][1:], lines[2 * i + 1]) for i in range(ds.n_reads)]
    fq_text = host.fastq_text(pairs)
    d.fq_bgzf, d.fq_gzip = str(d.dir / "bgzf.fastq.gz"), str(d.dir / "gzip.fastq.gz")
    open(d.fq_bgzf, "wb").write(host.bgzf(fq_text, list(range(65280, len(fq_text), 65280))))
    open(d.fq_gzip, "wb").write(gzip.compress(fq_text, 6))
    # a duplicated name: read 7 once more behind the last read, name and bases - the later read takes the name, so every
    # overlap of read 7 is now one of read 3000
    d.fa_dup = str(d.dir / "dup.fasta")
    open(d.fa_dup, "wb").write(host.fasta_text(pairs + [pairs[7]], 80))
    # a primary file the tokeniser calls irregular (a line with fewer than 12 columns: the host readers skip it)
    d.paf_irregular = str(d.dir / "irregular.paf")
    open(d.paf_irregular, "wb").write(open(d.paf, "rb").read() + b"short\tline\n")
    # sensitive overlaps
    o = Oracle(ds.read_len, ds.overlaps, n_threads=4)
    assert o.initialize() == 0
    o.pass2()
    o.preprocess_chimeras()
    p = o.piles()
    ds.sensitive(p["alive"], p["begin"], p["end"])
    ds.write_paf(d.sens, sensitive=True, target_len=(p["end"] - p["begin"]).astype(np.uint32))
    return d


def run(d, args, names, tag, **env):
    """-> (stdout, stage lines and counts of stderr without their times, CSV, JSON), all of stderr"""
    prefix = str(d.dir / tag)
    e = dict(os.environ, RALA_DEVICE_SEQUENCES="1", RALA_HIP_TRACE="1", **env)
    e.pop("RALA_DEVICE_NAMES", None)
    if names:
        e["RALA_DEVICE_NAMES"] = "1"
    r = subprocess.run([d.exe, "-d", prefix] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-3000:]
    stages = [re.sub(r" \d+\.\d+ s$", "", x) for x in err.splitlines() if x.startswith("[rala::")]
    dumps = [open(prefix + x, "rb").read() if os.path.exists(prefix + x) else None for x in (".csv", ".json")]        # (-p writes none)
    assert (dumps[0] is None) == ("-p" in args)
    return (r.stdout, stages, dumps[0], dumps[1]), err


def on_and_off(d, args, tag, tables=1, **env):
    on, err_on = run(d, args, True, tag + "_on", **env)
    off, err_off = run(d, args, False, tag + "_off", **env)
    assert on == off
    assert len(on[0]) > 1000 and any("number of nodes" in x for x in on[1])
    assert "device sequence index" in err_on and "device sequence index" in err_off
    assert err_on.count("device name table") == tables and "device name table" not in err_off
    return on, err_on


INPUTS = {
    "fasta": lambda d: ([d.fa, d.paf], {}),
    "bgzf_fastq": lambda d: ([d.fq_bgzf, d.paf], {}),
    "gzip_fastq": lambda d: ([d.fq_gzip, d.paf], {"RALA_DEVICE_GZIP": "1"}),
    "duplicated_name": lambda d: ([d.fa_dup, d.paf], {}),
    "sensitive": lambda d: (["-s", d.sens, d.fa, d.paf], {}),
    "trimmed_reads": lambda d: (["-p", d.fa, d.paf], {}),
    "two_ranks": lambda d: (["--gpus", "2", "-s", d.sens, d.fa, d.paf], {"RALA_COMM": "local", "RALA_GPU_DEVICES": "0,0"}),
}


@pytest.mark.parametrize("what", sorted(INPUTS))
def test_same_output_with_the_switch_on_and_off(data, what):
    args, env = INPUTS[what](data)
    on_and_off(data, args, what, **env)


def test_an_irregular_overlap_file_goes_to_the_host_reader_on_the_adopted_table(data):
    """the tokeniser hands the file back; the host reader then runs on the table the device built (no host build: there are no
    strings to build it from) - and RALA_DEVICE_INGEST=0 the same way; the output is that of the regular file, whose extra
    line the host readers skip"""
    regular, _ = on_and_off(data, [data.fa, data.paf], "regular")
    irregular, _ = on_and_off(data, [data.fa, data.paf_irregular], "irregular")
    host_reader, _ = on_and_off(data, [data.fa, data.paf], "host_reader", RALA_DEVICE_INGEST="0")
    assert irregular[0] == regular[0] and irregular[2:] == regular[2:] and host_reader == regular


def test_the_switch_alone_changes_nothing(data):
    """without RALA_DEVICE_SEQUENCES there is no index to build from: RALA_DEVICE_NAMES=1 is not looked at"""
    out = {}
    for names in ("1", "0"):
        env = dict(os.environ, RALA_DEVICE_NAMES=names, RALA_HIP_TRACE="1")
        env.pop("RALA_DEVICE_SEQUENCES", None)
        r = subprocess.run([data.exe, data.fa, data.paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        err = r.stderr.decode()
        assert r.returncode == 0, err[-3000:]
        assert "device name table" not in err and "device sequence index" not in err
        out[names] = (r.stdout, [re.sub(r" \d+\.\d+ s$", "", x) for x in err.splitlines() if x.startswith("[rala::")])
    assert out["1"] == out["0"] and len(out["1"][0]) > 1000
