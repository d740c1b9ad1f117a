"""Host build of k_replay's walk (no GPU): strk_search.h states the walk over a locus's reads twice — read by read
(replay_walk_serial) and by events, 64 lanes at a time with the quiet reads between two events committed at once
(replay_walk_events, on the predicate replay_quiet that the kernel uses) — and tools/replay_walk_asan.cpp runs one against the
other on random loci.  The same program runs a million loci under AddressSanitizer + UBSan from tools/replay_walk_asan.sh."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_walk_by_events_ends_like_the_walk_read_by_read(tmp_path):
    """20 000 loci of 1-200 reads (estimates from 0 up, stored results equal to the start or off by up to +-3, reads without a
    stored result, empty results, pending tables, searches that miss or do not certify, feedback on and off, both passes): the
    same stop, next read, fraction bits and outputs.  The corpus must hold what the walk can get wrong: events and fraction
    resets at all, a locus without any event, and events at lane 0, at lane 63 and at the first lane of a second batch."""
    exe = tmp_path / "replay_walk"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "replay_walk_asan.cpp")], check=True)
    out = subprocess.run([str(exe), "20000", "7"], capture_output=True, text=True)
    print(out.stdout.strip())
    loci, reads, events, resets, errors, no_event, lane0, lane63, batch2 = (int(x) for x in out.stdout.split())
    assert out.returncode == 0 and loci == 20000 and reads > loci
    assert errors == 0
    assert events > 0
    assert resets > 0
    assert no_event >= 1
    assert lane0 >= 1 and lane63 >= 1 and batch2 >= 1
