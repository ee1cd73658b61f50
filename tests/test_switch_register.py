"""The register of environment switches ("A/B switches") against the code: every CHORE_* variable the
library or bench.py reads has a row, every row names something that is read, and the switches retired in round 8 are read
nowhere.  Text only: no GPU, no import of the package."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"(CHORE_[A-Z0-9_]+)"
C_READ = re.compile(r'getenv\(\s*"' + NAME + '"')
PY_READS = [re.compile(r'os\.environ\.get\(\s*["\']' + NAME + r'["\']'),
            re.compile(r'os\.environ\[\s*["\']' + NAME + r'["\']\s*\]'),
            re.compile(r'["\']' + NAME + r'["\']\s+in\s+os\.environ')]

# removed in round 8 with the code only they reached (each had lost its measurement: DESIGN.md sections 4, 5 and 7)
RETIRED = ["CHORE_ENC_GROUPS", "CHORE_ENC_CHILD_FIRST", "CHORE_WGRAD_DBG", "CHORE_WGRAD128_WGS", "CHORE_QUERY_W8",
           "CHORE_QUERY_X3_BWD_SMALL", "CHORE_CONV_MW_LDS_MIN", "CHORE_CONV_MW_SKIP", "CHORE_CONV_RW_CUS", "CHORE_CONVGN_SIDE",
           "CHORE_FIT_TWO_STREAMS", "CHORE_FIT_SPLIT_RULE", "CHORE_PIPE_PRIO", "CHORE_FIT_CHAINS", "CHORE_SCATTER_SCAN"]


def _text(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def names_read():
    """{name: [files that read it]}"""
    found = {}
    csrc = os.path.join(ROOT, "chore_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        for n in C_READ.findall(_text(path)):
            found.setdefault(n, []).append(os.path.relpath(path, ROOT))
    py = sorted(glob.glob(os.path.join(ROOT, "chore_amd", "**", "*.py"), recursive=True)) + [os.path.join(ROOT, "bench.py")]
    for path in py:
        text = _text(path)
        for rx in PY_READS:
            for n in rx.findall(text):
                found.setdefault(n, []).append(os.path.relpath(path, ROOT))
    return found


def table_entries():
    """the names in the first column of the switch table; an entry ending in * covers every name with that prefix"""
    text = _text(os.path.join(ROOT, "DESIGN.md"))
    start = text.index("### A/B switches")
    rows = []
    for line in text[start:].splitlines()[1:]:
        if rows and not line.startswith("|"):          # the first table under the heading (the list of removed switches follows it)
            break
        if line.startswith("|") and not line.startswith("|---"):
            rows.append(line.split("|")[1])
    return set(re.findall(r"CHORE_[A-Z0-9_]+\*?", " ".join(rows)))


def _covers(entry, name):
    return name.startswith(entry[:-1]) if entry.endswith("*") else name == entry


def test_every_switch_read_is_in_the_register():
    read, table = names_read(), table_entries()
    assert len(read) > 40 and len(table) > 40          # the scan found the code and the table
    missing = {n: f for n, f in read.items() if not any(_covers(e, n) for e in table)}
    assert not missing, "read by the code, no row in DESIGN.md section 5: %s" % missing


def test_every_register_entry_is_read_somewhere():
    read, table = names_read(), table_entries()
    stale = sorted(e for e in table if not any(_covers(e, n) for n in read))
    assert not stale, "rows of DESIGN.md section 5 that nothing reads: %s" % stale


def test_retired_switches_are_read_nowhere():
    read = names_read()
    back = {n: read[n] for n in RETIRED if n in read}
    assert not back, "retired in round 8, read again: %s" % back
