"""The down-sampling entry points' bindings: INTEGRATION.md's Rust struct and the ctypes struct against include/lcr.h, the symbols."""
import ctypes as C
import os
import re

from longcallr_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rust_and_ctypes_bindings_match_the_header(tmp_path):
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [re.sub(r"//[^\n]*", "", b) for b in re.findall(r"```rust(.*?)```", md, flags=re.S)]
    fns = set(re.findall(r"pub fn (lcr_\w+)", "".join(blocks)))
    assert {"lcr_set_downsample", "lcr_set_downsample_rows", "lcr_get_downsample"} <= fns & set(_lib.SYMBOLS)
    m = [re.search(r"pub struct lcr_downsample_info\s*\{(.*?)\}", b, flags=re.S) for b in blocks]
    m = [x for x in m if x]
    assert len(m) == 1
    fields = [(a, b.strip()) for a, b in re.findall(r"pub (\w+):\s*([^,}]+)", m[0].group(1))]
    assert [a for a, _ in fields] == ["n_regions", "n_rows", "region_applied", "sampled", "dev_sampled"]
    off, rust = 0, {}
    for name, ty in fields:      # C layout rules: i32 = 4 / 4, a pointer = 8 / 8
        assert ty in ("i32", "*const u8"), ty
        sz = 4 if ty == "i32" else 8
        off = (off + sz - 1) // sz * sz
        rust[name] = off
        off += sz
    rust_size = (off + 7) // 8 * 8
    lines = ['#include "lcr.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(){",
             'printf("size %zu\\n", sizeof(lcr_downsample_info));']
    lines += ['printf("%s %%zu\\n", offsetof(lcr_downsample_info, %s));' % (f, f) for f in rust]
    lines.append("return 0;}")
    src, exe = tmp_path / "off.c", tmp_path / "off"
    src.write_text("\n".join(lines))
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = {k: int(v) for k, v in (l.split() for l in os.popen(str(exe)).read().strip().split("\n"))}
    assert got.pop("size") == rust_size == C.sizeof(_abi.LcrDownsampleInfo)
    assert got == rust == {f: getattr(_abi.LcrDownsampleInfo, f).offset for f in rust}
