"""The layout of the structs of include/opv_demod.h as gcc sees it (sizeof and offsetof, printed by a small C program), and the
check of a ctypes mirror against it. CPU only."""
import ctypes as C
import subprocess

from amd_lib import ROOT


def header_layout(tmp_path, fields):
    """fields: {C type name: [field names]} -> {C type name: (size, {field name: offset})}, from one compiled program"""
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "opv_demod.h"}"', "int main(void){"]
    for st, fs in fields.items():
        src.append(f'printf("{st} %zu\\n", sizeof({st}));')
        src += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fs]
    src.append("return 0;}")
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "l")], capture_output=True, text=True, check=True).stdout.splitlines())
    return {st: (int(got[st]), {f: int(got[f"{st}.{f}"]) for f in fs}) for st, fs in fields.items()}


def check_ctypes_layout(tmp_path, cls, c_name, size, fields):
    """the ctypes class has exactly `fields`, in this order; gcc's size of `c_name` == the class's == `size`; gcc's offset of every
    field == the class's. -> {field name: offset}, for what a caller asserts on top (a number, another struct's offsets)"""
    assert [f[0] for f in cls._fields_] == fields
    got_size, offsets = header_layout(tmp_path, {c_name: fields})[c_name]
    assert got_size == C.sizeof(cls) == size
    for f in fields:
        assert offsets[f] == getattr(cls, f).offset, f
    return offsets
