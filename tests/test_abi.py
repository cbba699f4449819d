"""CPU-only checks of the C ABI: the library loads and exports every symbol include/az_amd.h declares,
and argument validation (no GPU call) maps to the reference's exceptions."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from alphazero_amd import _lib


def test_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    declared = set(re.findall(r"\b(az_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.SYMBOLS)
    assert L.az_version() >= 100


def test_constructor_errors_match_reference():
    L = _lib.lib()
    h = C.c_void_p()
    # othello.py:87-88 : odd board size
    with pytest.raises(ValueError, match="Board size must be even"):
        _lib.check(L.az_net_create(0, 5, 5, 16, C.byref(h)))
    # connect4.py:90-91 : smaller than 4x4
    with pytest.raises(ValueError, match="at least 4x4"):
        _lib.check(L.az_net_create(1, 3, 7, 16, C.byref(h)))
    cfg = _lib.EngineCfg(0, 8, 8, 4, 10, 0.03, 0.25, 5, 4, 0, 0, 1, 0, 4096, 128, 1024)
    # schedulers.py:29-30 : temp_min_step < temp_max_step
    with pytest.raises(ValueError, match="temp_min_step"):
        _lib.check(L.az_engine_create(C.byref(cfg), None, None, C.byref(h)))


def test_trainer_buffer_listing_is_declared_and_its_classes_match_python():
    """az_trainer_buffer (every allocation of a trainer by index: name, class, pointer, bytes) is declared, listed and exported; the
    AZ_TBUF_* numbers of the header are the positions of the names Python uses (_lib.TRAINER_BUFFER_CLASSES), 0 .. n - 1 without a gap;
    HipTrainStep reaches the listing; a null trainer is a ValueError, not a crash"""
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"\bint\s+az_trainer_buffer\s*\(\s*az_trainer\s*\*", hdr) and "az_trainer_buffer" in _lib.SYMBOLS
    classes = {name.lower(): int(num) for name, num in re.findall(r"#define\s+AZ_TBUF_([A-Z_]+)\s+(\d+)", hdr)}
    assert classes == {name: i for i, name in enumerate(_lib.TRAINER_BUFFER_CLASSES)}
    assert set(_lib.TRAINER_BUFFER_CLASSES) == {"parameter", "momentum", "running_stat", "hyper", "workspace"}
    src = open(os.path.join(ROOT, "alphazero_amd", "csrc", "az_train.hip")).read()
    assert set(re.findall(r"AZ_TBUF_[A-Z_]+", src)) == {"AZ_TBUF_" + n.upper() for n in _lib.TRAINER_BUFFER_CLASSES}
    # one allocation call in the whole file, and it sits in talloc's body: an allocation anywhere else would escape the listing
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"static int talloc\(.*?\n}\n", code, flags=re.S)
    assert body and len(re.findall(r"\bhipMalloc\w*\s*\(", code)) == 1 == len(re.findall(r"\bhipMalloc\s*\(", body.group(0)))
    from alphazero_amd.train_step import HipTrainStep
    assert callable(HipTrainStep.buffers) and callable(HipTrainStep.views)
    L = _lib.lib()
    name, cls, p, n = C.c_char_p(), C.c_int32(), C.c_void_p(), C.c_int64()
    with pytest.raises(ValueError, match="null argument"):
        _lib.check(L.az_trainer_buffer(None, 0, C.byref(name), C.byref(cls), C.byref(p), C.byref(n)))


def test_product_does_not_import_oracle():
    """the oracle is test infrastructure: nothing under alphazero_amd/ may reference it"""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "alphazero_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("CPU oracle", "").replace("the oracle", "").lower() or f.endswith((".hip", ".h")), f
                assert "liboracle" not in src and "az_oracle" not in src, f


def test_counter_files_are_used_only_for_the_tree_they_were_measured_on(tmp_path, monkeypatch):
    """bench.py takes profiles/traffic.json, mfma_counters.json, kstep_counters.json into its line only when their `csrc_sha` equals the
    hash of the sources the running library was built from (round-2 verdict: file reads replayed into the driver's line)"""
    import importlib
    import json
    import sys
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    from alphazero_amd import _lib
    h = _lib.csrc_tree_hash()
    assert len(h) == 16 and h == _lib.csrc_tree_hash()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    (prof / "traffic.json").write_text(json.dumps({"othello_32768": {"k_trunk": 1}, "csrc_sha": h}))
    d, why = bench.stamped("traffic.json")
    assert d and d["othello_32768"]["k_trunk"] == 1 and h in why
    (prof / "traffic.json").write_text(json.dumps({"othello_32768": {"k_trunk": 1}, "csrc_sha": "0" * 16}))
    d, why = bench.stamped("traffic.json")
    assert d is None and "dropped" in why
    assert bench.stamped("missing.json")[0] is None
    # a file stamped for one component (the network kernels) is judged by that component's sources alone
    hn = _lib.csrc_tree_hash("net")
    assert hn != h and hn != _lib.csrc_tree_hash("engine") and hn != _lib.csrc_tree_hash("train")
    (prof / "traffic.json").write_text(json.dumps({"othello_4096": {"k_trunk": 2}, "csrc_component": "net", "csrc_sha": hn}))
    d, why = bench.stamped("traffic.json")
    assert d and d["othello_4096"]["k_trunk"] == 2 and "net" in why
    (prof / "traffic.json").write_text(json.dumps({"othello_4096": {"k_trunk": 2}, "csrc_component": "net", "csrc_sha": h}))
    assert bench.stamped("traffic.json")[0] is None
