"""CPU: rala_hip_gzip_chain - the walk from chunk 0 through what the device found and counted in every chunk of a single-member
gzip stream (rala_amd/csrc/ingest_formats.h: gzip_chain_from_spans), the host's only defence against a `next` the device made
of an untrusted file - on handmade span arrays: the jobs and counters of a good chain, and every refusal."""
import pytest

from rala_amd import hip

NONE = 2 ** 64 - 1
END = 5000                  # the trailer's first byte


def chunks():
    """four chunks, a chain of three: chunk 0 passes the start of chunk 1 (refuted: decoding from there is invalid) and lands on
    chunk 2, which lands on chunk 3, whose final block ends in the byte in front of the trailer"""
    return {"starts": [80, 9001, 17003, 25006], "status": [0, 2, 0, 1], "next": [2, 0, 3, 0], "text": [1000, 0, 2000, 300],
            "refuted": [1, 0, 0, 0], "end_bit": [0, 0, 0, 8 * END - 5]}


def chain(c, end=END, isize=None):
    """isize None: that of the chain 0 -> 2 -> 3"""
    if isize is None:
        isize = (c["text"][0] + c["text"][2] + c["text"][3]) & 0xFFFFFFFF
    return hip.gzip_chain(c["starts"], c["end_bit"], c["text"], c["next"], c["status"], c["refuted"], end, isize)


def test_one_chunk():
    jobs, tm = hip.gzip_chain([80], [8 * END], [500], [0], [1], [0], END, 500)
    assert [a.tolist() for a in jobs] == [[80], [NONE], [0], [500]]
    assert (tm["chunks"], tm["chunks_with_candidate"], tm["chunks_confirmed"], tm["chunks_refuted"]) == (1, 0, 0, 0)
    assert tm["max_wave_text_bytes"] == 500 and tm["text_bytes"] == 500


def test_a_chain_of_three_skips_the_refuted_chunk():
    jobs, tm = chain(chunks())
    start_bit, stop_bit, text_off, text_n = (a.tolist() for a in jobs)
    assert start_bit == [80, 17003, 25006]
    assert stop_bit == [17003, 25006, NONE]
    assert text_off == [0, 1000, 3000] and text_n == [1000, 2000, 300]
    assert (tm["chunks"], tm["chunks_with_candidate"], tm["chunks_confirmed"], tm["chunks_refuted"]) == (4, 3, 2, 1)
    assert tm["max_wave_text_bytes"] == 2000 and tm["text_bytes"] == 3300


@pytest.mark.parametrize("name,field,at,value", [("next == c", "next", 2, 2), ("next < c", "next", 2, 1), ("next == n_chunks", "next", 2, 4),
                                                 ("next far beyond", "next", 0, 0xFFFFFFFF), ("status 2 on the chain", "status", 2, 2),
                                                 ("status 3 on the chain", "status", 2, 3), ("status 3 at chunk 0", "status", 0, 3),
                                                 ("a status there is not", "status", 3, 7)])
def test_what_does_not_lead_forward_is_refused(name, field, at, value):
    c = chunks()
    c[field][at] = value
    jobs, _ = chain(c, isize=3300)
    assert jobs is None, name


def test_status_3_off_the_chain_is_harmless():
    c = chunks()
    c["status"][1], c["starts"][1] = 3, NONE
    jobs, tm = chain(c)
    assert jobs is not None and jobs[2].tolist() == [0, 1000, 3000]
    assert tm["chunks_with_candidate"] == 2 and tm["chunks_confirmed"] == 2


@pytest.mark.parametrize("end_bit", [8 * END + 1, 8 * (END - 1), 0, NONE])
def test_a_final_block_that_does_not_end_in_front_of_the_trailer_is_refused(end_bit):
    c = chunks()
    for ok in (8 * END - 7, 8 * END):           # (the last byte's first bit and its last)
        c["end_bit"][3] = ok
        assert chain(c)[0] is not None
    c["end_bit"][3] = end_bit
    assert chain(c)[0] is None


def test_isize_is_the_text_size_modulo_2_32():
    c = chunks()
    for isize in (3299, 3301, 0):
        assert chain(c, isize=isize)[0] is None
    c["text"][2] = 2 ** 32 + 7
    jobs, tm = chain(c, isize=1307)
    assert jobs is not None and jobs[2].tolist() == [0, 1000, 2 ** 32 + 1007]
    assert tm["text_bytes"] == 2 ** 32 + 1307 and tm["max_wave_text_bytes"] == 2 ** 32 + 7
    assert chain(c, isize=3300)[0] is None


def test_no_chunk_is_no_chain():
    jobs, tm = hip.gzip_chain([], [], [], [], [], [], END, 0)
    assert jobs is None and tm["chunks"] == 0
    assert "rala_hip_gzip_chain" in hip.SYMBOLS
