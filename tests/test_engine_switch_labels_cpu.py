"""CPU: the "bits" / "launches" label of every engine switch, in dafne_amd/engine_options.py and in INTEGRATION.md's "Engine
switches" table, is the one tests/test_gpu_engine_switches.py holds the switch to on the GPU."""
import dataclasses
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _held():
    import test_gpu_engine_switches as t
    return set(t.BITS_1A) | {"rp_mfma16"}, set(t.LAUNCHES), set(t.WR_DEPENDENT)


def test_labels_in_engine_options_py():
    from dafne_amd.engine_options import EngineOptions
    bits, launches, wr_dependent = _held()
    src = open(os.path.join(ROOT, "dafne_amd", "engine_options.py")).read()
    for f in dataclasses.fields(EngineOptions):
        m = re.search(r"((?:^    #.*\n)+)    %s: bool = _switch\(" % f.name, src, re.M)
        assert m, f.name
        comment = " ".join(line.strip().lstrip("#").strip() for line in m.group(1).splitlines())
        label = comment
        if f.name in wr_dependent:                      # launches by themselves, bits through the layers conv_wr then takes
            assert label.startswith("launches") and "With conv_wr on also bits" in comment, f.name
        else:
            assert label.startswith("bits" if f.name in bits else "launches"), (f.name, label[:40])
            assert (f.name in bits) != (f.name in launches)


def test_labels_in_the_integration_table():
    from dafne_amd.engine_options import EngineOptions
    bits, launches, wr_dependent = _held()
    rows = {}
    for line in open(os.path.join(ROOT, "INTEGRATION.md")):
        m = re.match(r"\| `(DAFNE_[A-Z0-9_]+)` \| `([a-z0-9_]+)` \|.*\| ([^|]+) \|\s*$", line)
        if m:
            rows[m.group(2)] = (m.group(1), m.group(3).strip())
    assert sorted(rows) == sorted(f.name for f in dataclasses.fields(EngineOptions))
    for f in dataclasses.fields(EngineOptions):
        env, changes = rows[f.name]
        assert env == f.metadata["env"]
        if f.name in wr_dependent:
            assert changes.startswith("launches") and "with `conv_wr` on also bits" in changes, f.name
        else:
            assert changes.startswith("bits" if f.name in bits else "launches"), (f.name, changes[:40])
