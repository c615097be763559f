"""The crafted long-run blocks of tests/lz_run_cases.py through the table kernel's phase code on the host
(tools/hostwave/lz_table_main.cpp: a stand-alone program under AddressSanitizer and UBSan, nothing is loaded into Python), in its
three orders of the racing reads and writes, against zlib -- and its counting mode (--count: the turns of the build's write loops
with every part written by its sequence's thread, and with the parts of 16 / 32 / 64 entries or more written by the whole wave)
against turn counts worked out by hand for two of the blocks."""
import os
import re
import shutil
import subprocess

import pytest

from tests import deflate_writer as dw
from tests import lz_run_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "lz_table_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(ROOT, "tools", "hostwave", "lz_table_main.cpp"), "-lz"])
    return out


def test_crafted_long_runs_on_the_host_under_sanitizers(program, tmp_path):
    cases = rc.build()
    path = str(tmp_path / "runs.bgzf")
    with open(path, "wb") as f:
        f.write(b"".join(c.block for c in cases))
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=600)
    tail = r.stdout[-4000:] + r.stderr[-4000:]
    assert r.returncode == 0 and "FAILED" not in r.stdout and "crafted: ok" in r.stdout, tail
    line = next(l for l in r.stdout.splitlines() if l.startswith(path + ": ok"))
    g = re.search(r"blocks (\d+) \(\+ (\d+) malformed skipped, (\d+) above 0xFF00 handed over\)", line)
    good = sum(1 for c in cases if c.status == 0)
    assert tuple(int(v) for v in g.groups()) == (good, len(cases) - good, 0), line      # (zlib refuses the malformed one: the tokens kernel's business)
    # the long match in front of the block's start, as a sequence stream built into the program
    g = re.search(r"crafted long_match_past_the_start: status (\d+)", r.stdout)
    assert g and int(g.group(1)) == rc.BAD_DIST, tail


def _turns(stdout, path, block):
    line = next(l for l in stdout.splitlines() if l.startswith("%s block %d:" % (path, block)))
    g = re.search(r"sequences (\d+), bytes (\d+), turns by owner (\d+) \(literals (\d+) \+ matches (\d+)\)", line)
    owner = tuple(int(v) for v in g.groups())
    scheme = {int(a): (int(b), int(c), int(d)) for a, b, c, d in re.findall(r"LONG_RUN (\d+): turns (\d+), long parts (\d+), long bytes (\d+)", line)}
    return owner, scheme


def test_the_counting_mode_reports_the_turns_a_hand_computation_gives(program, tmp_path):
    blocks = []
    for d in (rc.stored_600(), rc.lane_0_and_63()):
        blocks.append(dw.bgzf(d.getvalue(), bytes(d.data)))
    path = str(tmp_path / "two.bgzf")
    with open(path, "wb") as f:
        f.write(b"".join(blocks))
    r = subprocess.run([program, "--count", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    # 600 stored bytes: the sequences [255 | 0], [255 | 0], [90 | 0] in one wave of one batch.  Each by its own thread: the wave runs
    # as long as its longest literal part, 255 turns, and no match turn.  All three parts are long at 16, 32 and 64: ceil(255 / 64)
    # + ceil(255 / 64) + ceil(90 / 64) = 4 + 4 + 2 turns of the whole wave and no turn of a single thread.
    owner, scheme = _turns(r.stdout, path, 0)
    assert owner == (3, 600, 255, 255, 0)
    assert scheme == {16: (10, 3, 600), 32: (10, 3, 600), 64: (10, 3, 600)}
    # sequences 0: [1 | 100], 1 .. 63: [0 | 3] (the first wave), 64 .. 126: [0 | 3], 127: [0 | 200] (the second): 1 + 100 + 63 x 3 + 63 x 3 +
    # 200 = 679 bytes.  Each by its own thread: 1 + 100 turns in the first wave, 0 + 200 in the second, which the batch waits for.
    # With the two long matches by the wave: the first wave 1 (literal) + 3 (the short matches) + ceil(100 / 64) = 6 turns, the second
    # 0 + 3 + ceil(200 / 64) = 7.
    owner, scheme = _turns(r.stdout, path, 1)
    assert owner == (128, 679, 200, 0, 200)
    assert scheme == {16: (7, 2, 300), 32: (7, 2, 300), 64: (7, 2, 300)}
