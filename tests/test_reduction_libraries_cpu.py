"""CPU: what the nine handle-less reduction libraries are held to alike, stated once.  Two tests run per row of
reduction_libraries.LIBRARIES, with the short name as the id, and hold the row's library to the strictest form any of the
nine copies had: what the library links and what its two units include, call and leave alone; and the compiler's resource
remarks with the Makefile lines that build it.  What holds between the libraries -- no name twice, the order of
abi.LIBRARIES -- is asserted once for all of them, below.  The header against the library and the binding table, the header
as C, the kernel inventory and the stand-alone check program are still held in every tests/test_f32_x_cpu.py."""
import itertools
import os
import re

import pytest

import kernel_inventory
from kernel_inventory import unit_text
from native import CSRC, INCLUDE, declared, needed, remarks, undefined
from reduction_libraries import LIBRARIES, built, header, lib_path, signatures

each_library = pytest.mark.parametrize("x", list(LIBRARIES))


@each_library
def test_library_links_hip_alone_and_reads_no_environment(x):
    """The library is loaded with the HIP runtime and with nothing of torch, the oracle or the other libraries; its units
    read no environment, include nothing but their own two headers and specan.h, launch as often as the row says, keep
    clear of the row's words, and send both entry points through the one check."""
    row = LIBRARIES[x]
    built(x)
    libs = needed(lib_path(x))
    for other in ("torch", "oracle", "specan_hip", *(f"specan_{y}" for y in LIBRARIES if y != x)):
        assert other not in libs, libs
    assert "amdhip64" in libs
    assert "getenv" not in undefined(lib_path(x))
    kernel_unit, check_unit = row["units"]
    text = unit_text(kernel_unit) + unit_text(check_unit)
    assert all(name in text for name in row["names"]) and f"sa_{x}_check_call" in text
    assert "getenv" not in text and "environ" not in text.replace("environment", "")
    # the units include nothing of the chains or of the other reductions
    assert not re.search(r'#\s*include\s+"(?!sa_%s\.hpp|\.\./\.\./include/specan_%s\.h|specan\.h)' % (x, x), text), text[:200]
    code = re.sub(r"//.*", "", open(os.path.join(CSRC, kernel_unit)).read())
    for allowed in row.get("comment", ()):
        code = code.replace(allowed, "")
    for word in row["absent"]:
        assert word not in code, word
    for word, count in row.get("counts", {}).items():
        assert code.count(word) == count, word
    if row["fp_contract_off"]:
        assert "#pragma clang fp contract(off)" in code
    assert len(re.findall(r"hipLaunchKernelGGL", code)) == row["launches"] and "extern __shared__" not in code
    # the one check behind both entry points
    assert len(re.findall(r"sa_%s_check_call\(" % x, unit_text(check_unit))) >= 2
    assert len(re.findall(r"sa_%s_check_call\(" % x, code)) == 1


def figures(unit):
    """[(mangled function, {figure: value})] of a unit's resource remarks, in their order"""
    out = []
    for ln in remarks(unit).splitlines():
        name, figure = re.search(r"remark: Function Name: (\S+)", ln), re.search(r"remark:\s+(.+?): (\d+) \[", ln)
        if name:
            out.append((name.group(1), {}))
        elif figure and out:
            out[-1][1][figure.group(1)] = int(figure.group(2))
    return out


@each_library
def test_resource_remarks_show_no_scratch_and_no_spill(x):
    """The lines of the Makefile that build the library, spelled from the row; then the compiler's figures for its kernels,
    as `make resource-x-f32` prints them: the row's number of each, no scratch, no SGPR or VGPR spill, static LDS only and
    within the row's bounds.  VGPRs, occupancy and LDS are printed; the row's section of DESIGN.md records them."""
    row, X = LIBRARIES[x], x.upper()
    kernel_unit, check_unit = row["units"]
    make = open(os.path.join(CSRC, "Makefile")).read()
    for pin in (r"^%s_SRCS = %s %s$" % (X, re.escape(kernel_unit), re.escape(check_unit)), r"^%s_OBJS = " % X,
                r"^%s_OUT = \.\./libspecan_%s\.so$" % (X, x),
                r"^\$\(X_OUT\): \$\(X_OBJS\)\n\t\$\(HIPCC\) \$\(CXXFLAGS\) -shared \$\(X_OBJS\) -o \$@$".replace("X_", X + "_"),
                r"^all:.*\$\(%s_OUT\)" % X, r"^UNITS = .*\$\(%s_SRCS\)" % X, r"^clean:\n\trm .*\$\(%s_OUT\)" % X,
                r"^RESOURCE = .*resource-%s-f32" % x, r"^resource-%s-f32: UNITS = %s$" % (x, re.escape(kernel_unit))):
        assert re.search(pin, make, re.M), pin
    assert f"libspecan_{x}.so" in "\n".join(make.split("\n", 2)[:2])
    got = figures(kernel_unit)
    for kernel, (count, least, most) in row["remarks"].items():
        lds = [f["LDS Size [bytes/block]"] for name, f in got if kernel in name]
        assert len(lds) == count and all(least <= v <= most for v in lds), (kernel, lds)
    assert len(got) == sum(count for count, _, _ in row["remarks"].values()), [name for name, _ in got]
    for what in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill"):
        assert [f[what] for _, f in got] == [0] * len(got), what
    vgprs, occupancy = [f["VGPRs"] for _, f in got], [f["Occupancy [waves/SIMD]"] for _, f in got]
    print("FIGURE", x, "(DESIGN.md section %s)" % row["design"], "VGPRs", vgprs, "occupancy", occupancy,
          "LDS", [f["LDS Size [bytes/block]"] for _, f in got])
    if "occupancy" in row:
        assert occupancy == [row["occupancy"]] * len(got) and max(vgprs) <= row["vgprs_max"]
    assert "extern __shared__" not in unit_text(kernel_unit)


# ---------------------------------------------------------------------------------------------- between the libraries
def test_no_name_twice_and_the_order_of_the_rows():
    """Every pair among the binding tables is disjoint, and every pair among the headers' declared names; the tables are as
    large as they were; the rows of abi.LIBRARIES are those of the table here, in its order."""
    from fpga_real_time_fft_analyzer_amd import abi
    tables = [abi.SIGNATURES, abi.EXT_SIGNATURES] + [signatures(x) for x in LIBRARIES]
    headers = [os.path.join(INCLUDE, h) for h in ("specan.h", "specan_ext.h")] + [header(x) for x in LIBRARIES]
    for a, b in itertools.combinations(tables, 2):
        assert not set(a) & set(b), set(a) & set(b)
    for a, b in itertools.combinations(headers, 2):
        assert not set(declared(a)) & set(declared(b)), (a, b)
    assert [len(t) for t in tables] == [45, 5] + [4] * 9
    assert [sorted(signatures(x)) for x in LIBRARIES] == [row["names"] for row in LIBRARIES.values()]
    assert list(abi.LIBRARIES) == list(LIBRARIES)


def test_the_chain_library_holds_what_it_held():
    from fpga_real_time_fft_analyzer_amd import abi
    if not os.path.exists(abi.LIB_PATH):
        abi.build()
    assert kernel_inventory.inventory(abi.LIB_PATH) == set(kernel_inventory.TABLE)
