"""GPU: the -s file of a sharded run through one collective, rala_hip_mg_tokenise_sensitive - plain PAF and MHAP, BGZF, one
gzip member and five ragged members, over 1 / 2 / 3 / 8 ranks as threads on the one device (gzip_chunk_bytes 1024).  The shares
back to back are the host reader's columns without the length check (test_ingest_cpu.parse); what zlib refuses is the same
refusal on every rank and is followed by a good file on the same group.  (rala_hip_mg_run from such shares against the run from
host columns: tests/test_gpu_cli_ranks_gzip_members.py, whose -s file takes this entry.)"""
import struct

import numpy as np
import pytest

import test_gpu_bgzf as gb
import test_gpu_gzip_members as gm
import test_gpu_ranks_compressed as rc
import test_gpu_ranks_gzip_members as rm
import test_ingest_cpu as host

pytestmark = pytest.mark.gpu
COLLECTIVE = 2              # hp_text_device_ranks: the shares through rala_hip_mg_tokenise_sensitive


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """6000 lines as PAF and MHAP: plain, BGZF with ragged members, one gzip member, five ragged gzip members; the host reader's
    columns without the length check (one read's length is wrong on purpose: nobody may look)"""
    w = rm.World(tmp_path_factory.mktemp("rank_sens"), 6000, 12)
    w.wrong = np.array(w.lens, copy=True)
    w.wrong[5] += 1
    plain = {False: str(w.dir / "plain.paf"), True: str(w.dir / "as.mhap")}
    host._to_mhap(plain[False], plain[True])
    w.kinds, w.cols, w.five = {}, {}, {}
    for mhap in (False, True):
        text = open(plain[mhap], "rb").read()
        w.cols[mhap], bad = host.parse(plain[mhap], w.names, w.wrong, 2, 3 if mhap else True, check_lengths=False)
        assert bad == -1
        bgzf = plain[mhap] + ".bgzf.gz"
        gb.write_bgzf(plain[mhap], bgzf, gb.random_sizes(21 + mhap))
        starts = rm.line_starts(text)
        rng = np.random.default_rng(7 + mhap)
        texts = rm.cut(text, sorted(rng.choice(starts[1:], 4, replace=False).tolist()))
        w.five[mhap] = (texts, [rm.blocks(t) for t in texts])
        w.kinds[mhap] = {"plain": plain[mhap], "bgzf": bgzf, "one member": w.write("one", rm.blocks(text), mhap),
                         "five members": w.write("five", b"".join(w.five[mhap][1]), mhap)}
    return w


def shares(w, path, world, mhap, before=None, options=rm.MEMBERS):
    return rc.ranks(path, w.names, w.wrong, world, mhap=mhap, options=options, before=before, sensitive=COLLECTIVE, check_lengths=False)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("mhap", [False, True])
def test_shares_back_to_back_are_the_host_readers_columns(files, mhap, world):
    w = files
    for kind, path in w.kinds[mhap].items():
        got, irregular, bad, _, _, _ = shares(w, path, world, mhap)
        assert irregular == 0 and bad == -1, (kind, world, irregular)
        for f in w.cols[mhap]:
            assert len(got[f]) == len(w.cols[mhap][f]) and (got[f] == w.cols[mhap][f]).all(), (kind, world, f)


def test_refusals_are_the_same_on_every_rank_and_a_good_file_follows(files):
    w = files
    texts, m = w.five[False]
    good = b"".join(m)
    o2 = len(m[0]) + len(m[1])
    cases = {}
    b = bytearray(good)
    b[len(good) // 2] ^= 0x20
    cases["flip"] = bytes(b)
    b = bytearray(good)
    b[o2 - 8] ^= 1
    cases["crc_middle"] = bytes(b)
    cases["isize_last"] = good[:-4] + struct.pack("<I", len(texts[-1]) + 1)
    cases["between"] = m[0] + b"junk" + b"".join(m[1:])
    cases["cut"] = good[:len(good) * 2 // 3]
    cases["behind"] = good + b"\n"
    broken = bytearray(open(w.kinds[False]["bgzf"], "rb").read())
    broken[len(broken) * 3 // 4] ^= 0x5A
    for name, blob in cases.items():
        assert gm.zlib_takes(blob) is None, name
    cases["broken_bgzf"] = bytes(broken)
    for name, blob in cases.items():
        bad_path = w.write("sens_" + name, blob)
        for follow in ("five members", "plain"):
            # (hp_text_device_ranks marks a verdict that differs between ranks with a flag no rank gives)
            got, irregular, bad, _, _, was = shares(w, w.kinds[False][follow], 3, False, before=bad_path)
            assert was[0] == 8, (name, was)
            assert irregular == 0 and bad == -1, (name, follow)
            for f in w.cols[False]:
                assert (got[f] == w.cols[False][f]).all(), (name, follow, f)
    # the options off: a gzip file that is not BGZF is refused on every rank, BGZF and plain text are taken as they are
    for options in ({}, {"gzip_on_device": 1}, dict(rm.MEMBERS, gzip_members=0)):
        assert shares(w, w.kinds[False]["five members"], 3, False, options=options)[1] == 8, options
        for kind in ("plain", "bgzf"):
            got, irregular, _, _, _, _ = shares(w, w.kinds[False][kind], 3, False, options=options)
            assert irregular == 0 and (got["a_id"] == w.cols[False]["a_id"]).all(), (options, kind)
    got, irregular, _, _, _, _ = shares(w, w.kinds[False]["one member"], 3, False, options=dict(rm.MEMBERS, gzip_members=0))
    assert irregular == 0 and (got["b_end"] == w.cols[False]["b_end"]).all()
