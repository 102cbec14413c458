"""The environment knobs in the sources and in README.md's table name the same variables: every "FFTW_AMD_..." string
literal in fftw3_amd/csrc/*.c and *.hip is a row of the table under "Environment knobs", and every name in the table
that drives fa_read_knobs (planner.c: g_knob_table) is such a literal.  A consistency check of the documentation on
the project's own knob names, nothing more; no device, no library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fftw3_amd", "csrc")
LITERAL = re.compile(r'"(FFTW_AMD_[A-Z0-9_]+)"')


def _read(path):
    with open(path) as f:
        return f.read()


def _source_knobs():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.c")) + glob.glob(os.path.join(CSRC, "*.hip")):
        names.update(LITERAL.findall(_read(path)))
    return names


def _readme_table():
    section = _read(os.path.join(ROOT, "README.md")).split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    names = set()
    for line in section.splitlines():
        if line.startswith("| `FFTW_AMD_"):
            names.update(re.findall(r"`(FFTW_AMD_[A-Z0-9_]+)`", line.split("|")[1]))
    return names


def _reader_table():
    body = _read(os.path.join(CSRC, "planner.c")).split("g_knob_table[] = {", 1)[1].split("};", 1)[0]
    return LITERAL.findall(body)


def test_every_knob_in_the_sources_is_in_the_readme_table():
    assert len(_source_knobs()) > 20
    assert sorted(_source_knobs() - _readme_table()) == []


def test_the_reader_table_holds_source_knobs_once_each():
    names = _reader_table()
    assert names and len(set(names)) == len(names)
    assert set(names) <= _source_knobs()
    assert set(names) <= _readme_table()
