"""The library's build inputs: every unit of csrc/ is compiled, every header makes the library stale, and the training step stays
inside relu_field_kernels.hip -- the one file bench.py's traffic table (profiles/pmc_traffic.json) is tied to."""
import os
import re

from thr3ed_atom_amd import _lib

DEFINITION = re.compile(r"^(?:int|int32_t|int64_t|const char\*) (rf_[a-z_0-9]+)\(", re.M)


def units_on_disk():
    found = []
    for root, dirs, files in os.walk(_lib.CSRC_DIR):
        dirs[:] = [d for d in dirs if d != "tools"]
        found += [os.path.relpath(os.path.join(root, f), _lib.CSRC_DIR) for f in files if f.endswith(".hip")]
    return sorted(found)


def entry_points_of(unit):
    return set(DEFINITION.findall(open(os.path.join(_lib.CSRC_DIR, unit)).read()))


def test_every_unit_of_csrc_is_a_source():
    assert units_on_disk() == sorted(_lib.SOURCES)
    assert _lib.SOURCES[0] == "relu_field_kernels.hip"


def test_build_is_stale_after_any_source_or_header():
    inputs = _lib.build_inputs()
    assert all(os.path.isfile(p) for p in inputs)
    for name in _lib.SOURCES + ["rf_device.h"]:
        assert os.path.join(_lib.CSRC_DIR, name) in inputs
    assert os.path.join(_lib.INCLUDE_DIR, "relu_field.h") in inputs
    # (the list comes from the directory: a header added to csrc/ is covered without anybody remembering to name it)
    assert sorted(f for f in os.listdir(_lib.CSRC_DIR) if f.endswith(".h")) == sorted(os.path.basename(p) for p in inputs if p.endswith(".h") and os.path.dirname(p) == _lib.CSRC_DIR)


def test_every_entry_point_is_defined_once_and_the_train_step_stays_in_the_main_unit():
    defined = {unit: entry_points_of(unit) for unit in _lib.SOURCES}
    everything = [name for names in defined.values() for name in names]
    assert [everything.count(name) for name in _lib.EXPORTED_SYMBOLS] == [1] * len(_lib.EXPORTED_SYMBOLS)
    main = open(os.path.join(_lib.CSRC_DIR, "relu_field_kernels.hip")).read()
    body = main[main.index("int rf_train_step("):]
    body = body[:body.index("\n}\n")]  # the function's own closing brace (column 0)
    called = set(re.findall(r"\b(rf_[a-z_0-9]+)\(", body)) - {"rf_train_step"}
    assert {"rf_render_forward", "rf_render_backward_emit_direct", "rf_brick_accumulate_adam", "rf_brick_accumulate"} <= called
    assert called <= defined["relu_field_kernels.hip"]
    for unit in _lib.SOURCES[1:]:
        assert not (called & defined[unit]), f"{unit} defines an entry point of the training step"
