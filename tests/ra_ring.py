"""The ring variant of tiers.pyfg: the only real multi-robot range-aided fixture has four robots that all range each other
(agent graph K4, colours [0, 1, 2, 3]: a proper colouring never runs two agents at once), so the coloured-mode tests
filter it at run time into a problem whose agent graph is the 4-cycle A-B-C-D-A (colours [0, 1, 0, 1]).  Dropped: every
EDGE_RANGE line that joins robots A and C, joins robots B and D, or joins a pose of A to the landmark LC0.  The robot of a
symbol is its first letter; for 'L' followed by an upper-case letter it is that second letter."""
import gzip
import os

import common


def robot_of(symbol):
    if symbol[0] == "L" and len(symbol) > 1 and symbol[1].isupper():
        return symbol[1]
    return symbol[0]


def dropped(line):
    f = line.split()
    if not f or f[0] != "EDGE_RANGE":
        return False
    a, b = f[2], f[3]
    pair = {robot_of(a), robot_of(b)}
    if pair == {"A", "C"} or pair == {"B", "D"}:
        return True
    return (a[0] == "A" and b == "LC0") or (b[0] == "A" and a == "LC0")


def write_ring_variant(directory):
    """-> path of the variant (plain .pyfg) in `directory`, number of ranges kept, number dropped"""
    path = os.path.join(str(directory), "tiers_ring.pyfg")
    kept = gone = 0
    with gzip.open(os.path.join(common.DATA, "tiers.pyfg.gz"), "rt") as src, open(path, "w") as out:
        for line in src:
            if dropped(line):
                gone += 1
                continue
            kept += line.startswith("EDGE_RANGE")
            out.write(line)
    return path, kept, gone
