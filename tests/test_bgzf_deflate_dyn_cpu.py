"""bgzf_deflate_dyn_kernel (csrc/svx_deflate.hip: the encoder's parse with its tokens kept, Huffman codes built in the workgroup, the
smallest of stored, fixed and dynamic written) without a GPU: tools/hostwave/deflate_dyn_main.cpp runs the kernel's own phase code
(csrc/svx_deflate_core.hpp, encode_block_dyn) as loops over the workgroup's threads, in three orders (the file blocks: two) of the
racing table inserts, chain marks, histogram adds and bit writes, under AddressSanitizer and UBSan -- block, LDS arrays, workspace and
member in heap blocks of exactly their size.  Inputs: the crafted blocks of tests/deflate_enc_cases.py and tests/deflate_dyn_cases.py,
every 0xFF00-byte block of the straddling, long and decoy index-build files and the first eight of each golden BAM.  Every member is
checked with zlib and struct, against the fixed program's member of the same block (tools/hostwave/deflate_main.cpp) and, where it is
dynamic, by an own RFC 1951 decoder (deflate_dyn_cases.check_member); the sets' sizes against zlib level 1."""
import pytest

from tests import deflate_enc_cases as dc
from tests import deflate_dyn_cases as dy


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    """Both host programs on every block, once -> (cases, [(set, blocks)], per order (the members, the block types), the fixed
    program's members)."""
    d = tmp_path_factory.mktemp("deflate_dyn")
    cases, sets = dy.all_cases(), dy.file_sets(d)
    case_blocks, file_blocks = [c.data for c in cases], [b for _s, blocks in sets for b in blocks]
    per_order = dy.run_host(dy.build_host(d, "deflate_dyn_main", sanitize=True), d, "dyn_", case_blocks, file_blocks, 3, 2)
    (fixed, _stored), = dy.run_host(dy.build_host(d, "deflate_main"), d, "fix_", case_blocks, file_blocks, 1, 1)
    return cases, sets, per_order, fixed


def test_the_orders_agree_byte_for_byte(members):
    cases, sets, per_order, _fixed = members
    n_files = sum(len(blocks) for _s, blocks in sets)
    assert len(per_order[0][0]) == len(per_order[1][0]) == len(cases) + n_files and len(per_order[2][0]) == len(cases)
    assert per_order[0] == per_order[1]
    assert (per_order[0][0][:len(cases)], per_order[0][1][:len(cases)]) == per_order[2]


def test_crafted_blocks(members):
    """Every check of deflate_dyn_cases.check_member with the token streams decoded: the planted repeats under the built codes, the
    Fibonacci counts at the 15-bit limit, two distance codes of one bit where the block has no or one distance.

    The limit is asked of fibonacci_0 .. 2 (deflate_dyn_cases.fibonacci_tail_block), whose Fibonacci counts reach the code construction
    as literals: check_member measures Huffman's depth over their decoded tokens (above 15) and finds a 15-bit code.  Blocks of 22
    shuffled values with the counts 1 .. 17,711 (fibonacci_bytes_0 .. 2) are here too, with every other check, but cannot show the
    limit: the parse turns nine of their bytes in ten into matches, and the code over the tokens that remain is 13 bits deep."""
    cases, _sets, per_order, fixed = members
    got, btype = per_order[0]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    lengths, distances, seen = set(), set(), {0: 0, 1: 0, 2: 0}
    for c, m, t, f in zip(cases, got, btype, fixed):
        d = dy.check_member(m, c.data, t, f, c, tokens=True)
        seen[t] += 1
        if c.want_token is not None or getattr(c, "want_tokens", None):
            for l, dd in (d.matches if d is not None else dc.tokens(m[18:-8])[0] if t == 1 else []):
                lengths.add(l)
                distances.add(dd)
    assert set(dc.LENGTHS) <= lengths and set(dc.DISTANCES) <= distances
    assert min(seen.values()) > 0, seen                          # all three forms are written
    by_name = dict(zip(names, zip(got, btype)))
    assert by_name["empty"] == (dc.EOF_BLOCK, 1)
    assert by_name["tiny_300"][1] == 1 and by_name["random_0xFF00"][1] == 0 and len(by_name["random_0xFF00"][0]) == 65311
    for k in range(3):
        assert by_name["fibonacci_%d" % k][1] == 2


def test_file_blocks_and_their_size_against_zlib(members):
    """Every file block's member; a 15-bit code in at least one of them; and per set the members' bytes are not above what zlib
    level 1 (default strategy, the same 26 bytes a block) writes for the same blocks -- on the three random-base sets the bar is
    2.3 % above what unrestricted codes over these tokens would cost."""
    cases, sets, per_order, fixed = members
    at, deepest, report = len(cases), 0, []
    for name, blocks in sets:
        total = total_fixed = 0
        for k, block in enumerate(blocks):
            m, t, f = per_order[0][0][at], per_order[0][1][at], fixed[at]
            d = dy.check_member(m, block, t, f, dc.Case("%s[%d]" % (name, k), block))
            if d is not None:
                deepest = max(deepest, max(d.lit_lens))
            total, total_fixed, at = total + len(m), total_fixed + len(f), at + 1
        z1, z6 = dy.zlib_members(blocks, 1), dy.zlib_members(blocks, 6)
        report.append((name, len(blocks), sum(len(b) for b in blocks), total_fixed, total, z1, z6))
        print("%s: %d blocks, %d inflated, fixed %d, dynamic %d, zlib 1 %d, zlib 6 %d" % report[-1])
    assert deepest == 15
    for name, _n, n_in, total_fixed, total, z1, _z6 in report:
        assert total <= total_fixed and total < n_in, name
        assert total <= z1, (name, total, z1)
