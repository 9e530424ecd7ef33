"""The source text of thr3ed_atom_amd/csrc as the ABI tests read it (not a test module): comments stripped, a unit together with the
private headers it includes."""
import os
import re

from thr3ed_atom_amd import _lib

DEVICE_HEADER = "rf_device.h"  # (the render path's header: its atomics and LDS are the trainer's, no unit below inherits a claim from it)


def files():
    return sorted(f for f in os.listdir(_lib.CSRC_DIR) if f.endswith((".hip", ".h")))


def code(name: str) -> str:
    """one file of csrc/ without its comments"""
    text = open(os.path.join(_lib.CSRC_DIR, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def includes(name: str):
    return re.findall(r'#include\s+"([^"]+)"', code(name))


def private_headers(name: str):
    """the headers of csrc/ a file includes, directly or through them, DEVICE_HEADER left out, each once in include order"""
    found = []
    for header in includes(name):
        if header != DEVICE_HEADER and header not in found:
            found += [header] + [h for h in private_headers(header) if h not in found]
    return found


def unit_code(name: str) -> str:
    """a unit and its private headers (DEVICE_HEADER excepted), comments stripped: what a claim about the unit's code has to hold for"""
    return "\n".join(code(f) for f in private_headers(name) + [name])


def definitions(pattern: str):
    """[(file, match)] over all of csrc/: where ``pattern`` (a regular expression) occurs in code"""
    return [(f, m) for f in files() for m in re.findall(pattern, code(f))]
