"""CPU: rala_hip_gzip_chain_members - the walk through a gzip file of several members (rala_amd/csrc/ingest_formats.h:
gzip_chain_members) from what the device found and counted: chunk starts and spans as for one member, and the member header
candidates with the span decoded from each one's first block.  Handmade arrays: the jobs and the member list of good files
(two and three members, empty members anywhere, a candidate that is no header), every refusal, and on a one-member input the
jobs of rala_hip_gzip_chain."""
import copy

import pytest

from rala_amd import hip

import test_gzip_chain_cpu as one

NONE = 2 ** 64 - 1
JOB = 1000                  # compressed bytes a job of the handmade files takes


def build(members):
    """members: per member (the texts its jobs give, the CRC32 its trailer names); a member of no jobs' text - [0] - is an empty
    member of 12 deflate bits.  -> chunks, cands, file size, last CRC32 and ISIZE, and what the walk must give: jobs (start_bit,
    stop_bit, text_off, text_n, first) and members (text_off, text_n, crc).  The first member's first job is chunk 0, every
    other member's first job is a candidate's span, every later job of a member a chunk; behind every member lies a chunk
    without a start."""
    ch = {k: [] for k in ("starts", "end_bit", "text", "next", "status", "refuted")}
    cd = {k: [] for k in ("header_off", "deflate_bit", "prev_crc", "prev_isize", "end_bit", "text", "next", "status")}
    jobs, want_members = [], []
    p, text_at, prev = 0, 0, (0, 0)

    def chunk(start, end_bit, text, nxt, status):
        for k, v in zip(("starts", "end_bit", "text", "next", "status", "refuted"), (start, end_bit, text, nxt, status, 0)):
            ch[k].append(v)

    for m, (texts, crc) in enumerate(members):
        header, deflate = p, p + 10
        empty = texts == [0]
        starts = [8 * (deflate + JOB * i) + (i % 7 if i else 0) for i in range(len(texts))]
        end_bit = 8 * deflate + 10 if empty else 8 * (deflate + JOB * len(texts)) - 5
        trailer = (end_bit + 7) // 8
        for i, t in enumerate(texts):
            last = i == len(texts) - 1
            nxt = 0 if last else len(ch["starts"]) + (1 if i == 0 and m == 0 else 0 if i == 0 else 1)
            if i == 0 and m > 0:
                for k, v in zip(("header_off", "deflate_bit", "prev_crc", "prev_isize", "end_bit", "text", "next", "status"),
                                (header, starts[0], prev[0], prev[1], end_bit if last else 0, t, nxt, 1 if last else 0)):
                    cd[k].append(v)
            else:
                chunk(starts[i], end_bit if last else 0, t, nxt, 1 if last else 0)
            jobs.append((starts[i], NONE if last else starts[i + 1], text_at, t, 1 if i == 0 else 0))
            text_at += t
        chunk(NONE, 0, 0, 0, 3)
        want_members.append((text_at - sum(texts), sum(texts), crc))
        prev = (crc, sum(texts) & 0xFFFFFFFF)
        p = trailer + 8
    return ch, cd, p, prev[0], prev[1], jobs, want_members


def walk(ch, cd, file_n, crc, isize):
    return hip.gzip_chain_members(ch, cd, file_n, crc, isize)


def accepted(members):
    ch, cd, file_n, crc, isize, jobs, want = build(members)
    got, tm = walk(ch, cd, file_n, crc, isize)
    assert got is not None
    arrays, mem = got
    assert list(zip(*[a.tolist() for a in arrays])) == jobs
    assert mem == want
    assert tm["text_bytes"] == sum(t for _, t, _ in want) and tm["chunks_confirmed"] == len(jobs) - len(want)
    return ch, cd, file_n, crc, isize


TWO = [([1000, 2000, 300], 0x11111111), ([700, 50], 0x22222222)]
THREE = TWO + [([2 ** 32 + 5], 0x33333333)]
EMPTY = ([0], 0)


def test_the_symbol_is_exported():
    assert "rala_hip_gzip_chain_members" in hip.SYMBOLS and hasattr(hip.lib(), "rala_hip_gzip_chain_members")


def test_two_and_three_members():
    accepted(TWO)
    accepted(THREE)
    accepted([([5], 1), ([6], 2)])


@pytest.mark.parametrize("at", [0, 1, 2, 3])
def test_empty_members_in_front_in_the_middle_and_at_the_end(at):
    m = list(THREE)
    m.insert(at, EMPTY)
    accepted(m)
    accepted([EMPTY, EMPTY] + m + [EMPTY])


def test_a_false_candidate_is_never_reached():
    ch, cd, file_n, crc, isize, jobs, want = build(TWO)
    # a magic inside the first member's deflate bytes (decoding from there is invalid), and one that decodes to its own end
    for at, status, end_bit in ((0, 2, 0), (1, 1, 8 * 2500)):
        header = 1500 + 700 * at
        for k, v in zip(("header_off", "deflate_bit", "prev_crc", "prev_isize", "end_bit", "text", "next", "status"),
                        (header, 8 * (header + 10), 7, 7, end_bit, 9, 0, status)):
            cd[k].insert(at, v)
    got, _ = walk(ch, cd, file_n, crc, isize)
    assert got is not None and got[1] == want
    assert list(zip(*[a.tolist() for a in got[0]])) == jobs


def refused(ch, cd, file_n, crc, isize):
    got, _ = walk(ch, cd, file_n, crc, isize)
    assert got is None


def test_bytes_behind_a_trailer_that_are_no_candidate():
    ch, cd, file_n, crc, isize = accepted(TWO)
    for shift in (1, -1, 8):
        bad = copy.deepcopy(cd)
        bad["header_off"][0] += shift
        refused(ch, bad, file_n, crc, isize)
    refused(ch, {k: [] for k in cd}, file_n, crc, isize)
    refused(ch, cd, file_n + 1, crc, isize)             # a byte behind the last trailer


def test_a_wrong_inner_isize_and_a_wrong_last_one():
    ch, cd, file_n, crc, isize = accepted(THREE)
    for k in (0, 1):
        bad = copy.deepcopy(cd)
        bad["prev_isize"][k] ^= 1
        refused(ch, bad, file_n, crc, isize)
    refused(ch, cd, file_n, crc, isize ^ 1)
    accepted(THREE)                                      # (a text of 2^32 + 5 bytes: ISIZE 5)


def test_a_next_that_points_backwards():
    ch, cd, file_n, crc, isize = accepted(TWO)
    bad = copy.deepcopy(cd)
    bad["next"][0] = 1                                   # the second member's first span lands on a chunk of the first member
    refused(ch, bad, file_n, crc, isize)
    for nxt in (0, 1, len(ch["starts"]), 3):             # chunk 1's: itself, backwards, beyond the chunks, a chunk without a start
        bad = copy.deepcopy(ch)
        bad["next"][1] = nxt
        if nxt == 3:
            assert ch["starts"][3] == NONE
        refused(bad, cd, file_n, crc, isize)


def test_a_status_above_1_on_the_chain_and_a_cut_member():
    ch, cd, file_n, crc, isize = accepted(TWO)
    for status in (2, 3, 7):
        bad = copy.deepcopy(cd)
        bad["status"][0] = status
        refused(ch, bad, file_n, crc, isize)
    refused(ch, cd, file_n - 1, crc, isize)              # the last trailer is cut
    refused(ch, cd, file_n - 9, crc, isize)


def test_a_final_block_that_ends_short_of_the_last_trailer():
    ch, cd, file_n, crc, isize = accepted(TWO)
    last = max(k for k in range(len(ch["status"])) if ch["status"][k] == 1)
    for delta in (-16, -8, 8, 8 * 100):
        bad = copy.deepcopy(ch)
        bad["end_bit"][last] += delta
        refused(bad, cd, file_n, crc, isize)
    bad = copy.deepcopy(ch)
    bad["end_bit"][last] = 0                             # an end in front of the job's own start
    refused(bad, cd, file_n, crc, isize)


def test_one_member_gives_the_jobs_of_rala_hip_gzip_chain():
    c = one.chunks()
    want, tm1 = one.chain(c)
    ch = {"starts": c["starts"], "end_bit": c["end_bit"], "text": c["text"], "next": c["next"], "status": c["status"], "refuted": c["refuted"]}
    none = {k: [] for k in ("header_off", "deflate_bit", "prev_crc", "prev_isize", "end_bit", "text", "next", "status")}
    first = {"header_off": [0], "deflate_bit": [80], "prev_crc": [0], "prev_isize": [0], "end_bit": [0], "text": [1000], "next": [2], "status": [0]}
    for cd in (none, first):
        got, tm = walk(ch, cd, one.END + 8, 0xABCDEF01, 3300)
        assert got is not None
        for a, b in zip(got[0][:4], want):
            assert a.tolist() == b.tolist()
        assert got[0][4].tolist() == [1, 0, 0] and got[1] == [(0, 3300, 0xABCDEF01)]
        for k in ("chunks", "chunks_with_candidate", "chunks_confirmed", "chunks_refuted", "max_wave_text_bytes", "text_bytes"):
            assert tm[k] == tm1[k], k
    assert walk(ch, none, one.END + 8, 0, 3301)[0] is None
