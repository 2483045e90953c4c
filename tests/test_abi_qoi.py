"""No device: the subdomain and reaction objectives at the ABI boundary -- their symbols are declared, exported and bound,
the two descriptors have the layout of the ctypes mirror (the header compiled by gcc and g++), null arguments are refused
before anything is touched, and the Python names pass their arguments on and record the objective."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["c8_set_qoi_subdomain", "c8_set_qoi_reaction"]
LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "c8.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(c8_subdomain_qoi_desc), offsetof(c8_subdomain_qoi_desc, kind), offsetof(c8_subdomain_qoi_desc, elem_set),
         offsetof(c8_subdomain_qoi_desc, index));
  printf("%zu %zu %zu %zu %zu\n", sizeof(c8_reaction_desc), offsetof(c8_reaction_desc, coord_idx), offsetof(c8_reaction_desc, coord_value),
         offsetof(c8_reaction_desc, coord_tol), offsetof(c8_reaction_desc, reaction_comp));
  printf("%d %d %d\n", C8_QOI_AVG_STRESS, C8_QOI_AVG_LOCAL_VAR, C8_QOI_DISP_COMP);
  return 0;
}
"""


def header():
    return open(os.path.join(ROOT, "include", "c8.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from calibr8_amd import lib
    L = lib.load_library()
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    bound = {s[0]: s for s in lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == 2, name


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_descriptors_match_the_ctypes_mirror(tmp_path, compiler, std, ext):
    from calibr8_amd import lib
    src, exe = tmp_path / ("layout." + ext), tmp_path / "layout"
    src.write_text(LAYOUT)
    subprocess.check_call([compiler, std, "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sub, rea, enums = [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    S, R = lib.SubdomainQoiDesc, lib.ReactionDesc
    assert [f[0] for f in S._fields_] == ["kind", "elem_set", "index"]
    assert [f[0] for f in R._fields_] == ["coord_idx", "coord_value", "coord_tol", "reaction_comp"]
    assert sub == [C.sizeof(S), S.kind.offset, S.elem_set.offset, S.index.offset]
    assert rea == [C.sizeof(R), R.coord_idx.offset, R.coord_value.offset, R.coord_tol.offset, R.reaction_comp.offset]
    assert enums == [lib.C8_QOI_AVG_STRESS, lib.C8_QOI_AVG_LOCAL_VAR, lib.C8_QOI_DISP_COMP] == [0, 1, 2]


def test_null_arguments_are_refused():
    from calibr8_amd import lib
    L = lib.load_library()
    never_read = C.cast(C.create_string_buffer(8), C.c_void_p)     # stands for a context; the refusals come first
    assert L.c8_set_qoi_subdomain(None, C.byref(lib.SubdomainQoiDesc(0, 0, 0))) == lib.C8_ERR_ARG and b"c8_set_qoi_subdomain" in L.c8_last_error()
    assert L.c8_set_qoi_subdomain(never_read, None) == lib.C8_ERR_ARG and b"c8_set_qoi_subdomain" in L.c8_last_error()
    assert L.c8_set_qoi_reaction(None, C.byref(lib.ReactionDesc(1, 0.0, 1e-8, 1))) == lib.C8_ERR_ARG and b"c8_set_qoi_reaction" in L.c8_last_error()
    assert L.c8_set_qoi_reaction(never_read, None) == lib.C8_ERR_ARG and b"c8_set_qoi_reaction" in L.c8_last_error()


class _Recorder:
    """stands for the library behind an Assembler: records the descriptors of the two setters"""

    def __init__(self):
        self.calls = []

    def c8_set_qoi_subdomain(self, h, d):
        d = d._obj
        self.calls.append(("subdomain", d.kind, d.elem_set, d.index))
        return 0

    def c8_set_qoi_reaction(self, h, d):
        d = d._obj
        self.calls.append(("reaction", d.coord_idx, d.coord_value, d.coord_tol, d.reaction_comp))
        return 0


def test_python_names_pass_the_descriptors_on_and_record_the_objective():
    from calibr8_amd import Assembler, lib, local_dof
    asm = Assembler.__new__(Assembler)       # no device: the methods under test only pass their arguments on
    asm.L, asm.h, asm.local_type, asm.nloc = _Recorder(), None, "hypo_hill_plane_stress", 5
    asm.set_qoi_subdomain("avg_stress", 1, 7)
    assert asm.objective == ("subdomain", lib.C8_QOI_AVG_STRESS, 1, 0)
    asm.set_qoi_subdomain("avg_local_var", 0, "alpha")
    assert asm.objective == ("subdomain", lib.C8_QOI_AVG_LOCAL_VAR, 0, 3)
    asm.set_qoi_subdomain(lib.C8_QOI_DISP_COMP, 2, 1)
    assert asm.objective == ("subdomain", lib.C8_QOI_DISP_COMP, 2, 1)
    asm.set_qoi_reaction(coord_idx=0, coord_value=0.5, coord_tol=1e-6, comp=2)
    assert asm.objective == ("reaction", 0, 0.5, 1e-6, 2)
    assert asm.L.calls == [("subdomain", 0, 1, 7), ("subdomain", 1, 0, 3), ("subdomain", 2, 2, 1), ("reaction", 0, 0.5, 1e-6, 2)]
    # alpha is the last local unknown but for the two hypo_hill plane rows; the elastic models have none
    assert local_dof("small_J2", 7, "alpha") == 6 and local_dof("hyper_J2_plane_stress", 6, "alpha") == 5
    assert local_dof("hypo_hill_plane_strain", 5, "alpha") == 3
    for bad in (("elastic", 1, "alpha"), ("small_J2", 7, "pstrain")):
        with pytest.raises(ValueError):
            local_dof(*bad)
    with pytest.raises(KeyError):
        asm.set_qoi_subdomain("von_mises", 0)
