"""The scene tables equal the parent commit's, word for word.

tools/tables_digest.py evaluates mrt_debug_tables_digest (mrt_tables.hip: FNV-1a 64 over each table's
length and bytes, then the scalars) for reference scenes 0-9 and every entry of the synthetic
catalogue, with no test hook set and with each of MRT_NO_BVHW, MRT_FORCE_GENERIC and MRT_NO_SIG set;
tests/golden/tables_parent.json is its output on the parent commit's build (the commit it names), made
before the builder moved into its own unit and was split into stages.  A view the builder refuses is
refused in both with the same mrt_last_error text.  No GPU: the builder is host code.
"""
import json
import os
import sys

import pytest

import test_synthetic_scenes as tss
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tables_digest as td  # noqa: E402

with open(os.path.join(GOLDEN, "tables_parent.json")) as _f:
    PARENT = json.load(_f)["cases"]

_scenes = {}


def scene_of(mrt, name):
    if name not in _scenes:
        if name.startswith("scene_"):
            _scenes[name] = tss.ref_scene(mrt, int(name[6:]))
        else:
            _scenes[name] = tss.built(mrt, next(e for e in tss.CATALOGUE if e.name == name))[0]
    return _scenes[name]


NAMES = [f"scene_{i}" for i in range(10)] + tss.IDS


def test_fixture_covers_every_case():
    assert sorted(PARENT) == sorted(NAMES)
    assert all(sorted(PARENT[n]) == sorted(td.SETTINGS) for n in NAMES)
    # the hooks reach the builder: each changes the tables of some scene
    for h in td.HOOKS:
        assert any(PARENT[n][h] != PARENT[n]["none"] for n in NAMES), h


@pytest.mark.parametrize("setting", td.SETTINGS)
@pytest.mark.parametrize("name", NAMES)
def test_tables_equal_parent(mrt, monkeypatch, name, setting):
    s = scene_of(mrt, name)
    for h in td.HOOKS:
        monkeypatch.delenv(h, raising=False)
    if setting != "none":
        monkeypatch.setenv(setting, "1")
    got = td.digest(mrt, s)
    assert got == PARENT[name][setting], (name, setting)
