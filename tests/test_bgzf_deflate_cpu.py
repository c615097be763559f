"""bgzf_deflate_kernel (csrc/svx_deflate.hip: one workgroup turns a block of up to 0xFF00 bytes into a BGZF member, fixed Huffman
code or stored) without a GPU: tools/hostwave/deflate_main.cpp runs the kernel's own phase code (csrc/svx_deflate_core.hpp) as loops
over the workgroup's threads, in three orders (the file blocks: two) of the racing table inserts, chain marks and bit writes, under AddressSanitizer and
UBSan -- block, LDS arrays and member in heap blocks of exactly their size.  Inputs: tests/deflate_enc_cases.py (crafted blocks) and
the 0xFF00-byte blocks of the inflated golden BAMs and of the index-build files.  Every member is checked with zlib and struct
(deflate_enc_cases.check_member), the planted repeats are looked up in the members' token streams.  And the header rewrite of
svision_amd/sort.py."""
import struct

import numpy as np
import pytest

from tests import htslike
from tests import deflate_enc_cases as dc

@pytest.fixture(scope="module")
def members(tmp_path_factory):
    """The host program on every case, once -> (cases, [(name, block)] of the files, per order (the members, the stored flags)).  The
    crafted cases run in three orders, the file blocks -- 25 MB -- in two."""
    d = tmp_path_factory.mktemp("deflate")
    cases, files = dc.crafted(), dc.bam_blocks(d)
    return cases, files, dc.run_host(dc.build_host(d, sanitize=True), d, cases, files, 3, 2)


def test_the_orders_agree_byte_for_byte(members):
    cases, files, per_order = members
    assert len(per_order[0][0]) == len(per_order[1][0]) == len(cases) + len(files) and len(per_order[2][0]) == len(cases)
    assert per_order[0] == per_order[1]
    assert (per_order[0][0][:len(cases)], per_order[0][1][:len(cases)]) == per_order[2]


def test_crafted_blocks_against_zlib(members):
    cases, _files, per_order = members
    got, stored = per_order[0]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c, m, s in zip(cases, got, stored):
        assert dc.check_member(m, c.data, c) == bool(s), c.name
    by_name = dict(zip(names, got))
    assert by_name["empty"] == dc.EOF_BLOCK == htslike.EOF_BLOCK
    assert len(by_name["random_0xFF00"]) == 65311
    assert len(by_name["equal_0xFF00"]) <= 512
    # bit order: the literal 'A' = 0x41 is the code 0x30 + 0x41 = 0111 0001, first bit first behind the 3 header bits
    bits = np.unpackbits(np.frombuffer(by_name["bytes_1"][18:-8], np.uint8), bitorder="little")
    assert bits[:3].tolist() == [1, 1, 0] and bits[3:11].tolist() == [0, 1, 1, 1, 0, 0, 0, 1] and not bits[11:18].any()


def test_planted_repeats_are_carried_with_their_codes(members):
    """Every length and distance code boundary shows up in a member's token stream, extra bits included (tokens() decodes them least
    significant bit first; zlib has inflated the same stream to the input)."""
    cases, _files, per_order = members
    lengths, distances = set(), set()
    for c, m in zip(cases, per_order[0][0]):
        if c.want_token is not None and m[18] & 7 == 3:
            for l, d in dc.tokens(m[18:-8])[0]:
                lengths.add(l)
                distances.add(d)
    assert set(dc.LENGTHS) <= lengths and set(dc.DISTANCES) <= distances


def test_file_blocks_against_zlib(members):
    cases, files, per_order = members
    got = per_order[0][0][len(cases):]
    assert len(files) > 20 and sum(len(b) == dc.BLOCK for _n, b in files) > 15
    total_in = total_out = 0
    for (name, block), m in zip(files, got):
        c = dc.Case(name, block)
        dc.check_member(m, block, c)
        total_in, total_out = total_in + len(block), total_out + len(m)
    assert total_out < total_in                                  # BAM records do compress under the fixed code


# ---- the header rewrite of svision_amd/sort.py
def test_header_rewrite():
    from svision_amd import sort
    sq = "@SQ\tSN:chrA\tLN:400000\n@PG\tID:aligner\tPN:aligner\n"
    assert sort.sorted_header_text("@HD\tVN:1.5\tSO:unsorted\n" + sq) == "@HD\tVN:1.5\tSO:coordinate\n" + sq
    assert sort.sorted_header_text(sq) == "@HD\tVN:1.6\tSO:coordinate\n" + sq
    assert sort.sorted_header_text("") == "@HD\tVN:1.6\tSO:coordinate\n"
    assert sort.sorted_header_text("@HD\tVN:1.6\tSO:queryname\tGO:query\tSS:queryname:natural\tXX:kept\n" + sq) == "@HD\tVN:1.6\tSO:coordinate\tXX:kept\n" + sq
    assert sort.sorted_header_text("@HD\tVN:1.4\n" + sq) == "@HD\tVN:1.4\tSO:coordinate\n" + sq
    assert sort.sorted_header_text("@HD\tSO:unknown\n" + sq) == "@HD\tVN:1.6\tSO:coordinate\n" + sq
    assert "@PG" not in sort.sorted_header_text("@SQ\tSN:a\tLN:1\n")


def test_header_bytes_keep_the_dictionary():
    from svision_amd import sort
    text = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrA\tLN:7\n\0\0"
    refs = struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrA\0" + struct.pack("<i", 7)
    out = sort.sorted_header_bytes(b"BAM\x01" + struct.pack("<i", len(text)) + text + refs)
    new = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:7\n"
    assert out == b"BAM\x01" + struct.pack("<i", len(new)) + new + refs
    with pytest.raises(sort.SortWriteError):
        sort.sorted_header_bytes(b"BAX\x01" + bytes(8))
    assert issubclass(sort.SortWriteError, ValueError)


def test_the_record_stream_is_sized_from_the_isize_fields(tmp_path):
    """sort_bam allocates the record stream once, before the pass: the members' ISIZE sum is the file's inflated bytes, and the bytes
    in front of the first record are the header's."""
    import os
    from svision_amd import index, sort
    from tests import baicases, helpers
    path = os.path.join(helpers.GOLDEN, "collect_small.bam")
    w = baicases.walk(path)
    assert sort.inflated_size(path) == len(w.stream)
    raw = open(path, "rb").read()
    assert [(at, n) for at, n, _x, _i in index.bgzf_members(path)][-1] == (len(raw) - 28, 28)      # the end-of-file marker: 28 bytes, ISIZE 0
    for cut in (len(raw) - 29, len(raw) - 5, 7):                 # a member without its end, a footer cut, not even a header
        p = str(tmp_path / ("cut%d.bam" % cut))
        with open(p, "wb") as f:
            f.write(raw[:cut])
        with pytest.raises(sort.SortWriteError):
            sort.inflated_size(p)
    p = str(tmp_path / "nobc.bam")
    with open(p, "wb") as f:
        f.write(raw[:12] + b"XY" + raw[14:])                     # the extra field without a BC subfield
    with pytest.raises(sort.SortWriteError):
        sort.inflated_size(p)
