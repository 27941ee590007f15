"""The workspaces of the radix sort's users do not grow.

The six *_workspace_bytes functions are host-only. The literals below are what they returned before the sort's scratch got its one
description in csrc/radix.h (SortScratch, sort_scratch_bytes), over shapes on both sides of every chunk-size switch of rs_chunk
(sorted rows just below and above 2^21 and 2^22), the smallest shapes each function accepts, and the shapes of the benchmarks
(the 70k, 250k and 1M meshes and their face soups; 512 x 512 pixels at B = 1 and 8; 8 x 1024 x 1024 for the texture lookup).
A layout change may shrink a workspace; it must not make a caller allocate more.
"""
import ctypes

import pytest

from largesteps import _native

BEFORE = {
    "ls_remove_duplicates_workspace_bytes": [
        ((0,), 2756), ((1,), 2780), ((2,), 2804), ((1000,), 26756), ((2097151,), 54530728), ((2097152,), 54530752), ((2097153,), 52435676),
        ((4194303,), 104866472), ((4194304,), 104866496), ((4194305,), 102771420), ((423360,), 11010044), ((1500000,), 39003956),
        ((5991360,), 146801272),
    ],
    "ls_csr_transpose_workspace_bytes": [
        ((1, 0,), 2956), ((1, 1,), 2968), ((1000, 6994,), 103180), ((5, 2097153,), 27270056), ((4194304, 7,), 16788444),
        ((70000, 2097151,), 29645112), ((70000, 2097152,), 29645124), ((70000, 2097153,), 27550036), ((70000, 4194303,), 54815032),
        ((70000, 4194304,), 54815044), ((70000, 4194305,), 52719956), ((70562, 493922,), 7200364), ((250002, 1750002,), 25504384),
        ((998562, 6989922,), 91383804),
    ],
    "ls_corner_ranks_workspace_bytes": [
        ((0, 2,), 2960), ((1, 2,), 3008), ((100, 52,), 7960), ((699050, 349527,), 39151808), ((699051, 349527,), 37056756),
        ((1398101, 699052,), 74108452), ((1398102, 699053,), 72013404), ((141120, 70562,), 7905608), ((500000, 250002,), 28004160),
        ((1997120, 998562,), 102864836), ((0, 0,), 2952), ((10, 4194304,), 16788840),
    ],
    "ls_raster_workspace_bytes": [
        ((1, 0, 1, 1, 0,), 4608), ((1, 1, 1, 1, 3,), 4864), ((1, 100, 64, 64, 3,), 96000), ((1, 1000, 1024, 2047, 0,), 46162176),
        ((1, 1000, 1024, 2048, 3,), 46184704), ((1, 1000, 1025, 2047, 1,), 44109056), ((1, 1000, 2048, 2047, 3,), 88084736),
        ((1, 1000, 2048, 2048, 0,), 88127744), ((1, 1000, 2049, 2048, 4,), 86084608), ((2, 1048576, 16, 16, 3,), 92292608),
        ((1, 141120, 512, 512, 0,), 11978240), ((1, 141120, 512, 512, 3,), 11978240), ((8, 141120, 512, 512, 0,), 95816192),
        ((8, 141120, 512, 512, 3,), 95816192), ((1, 1997120, 512, 512, 0,), 93645824), ((1, 1997120, 512, 512, 3,), 93645824),
        ((8, 1997120, 512, 512, 0,), 749157120), ((8, 1997120, 512, 512, 3,), 749157120),
    ],
    "ls_raster_adjacency_workspace_bytes": [
        ((0,), 2204), ((1,), 2236), ((100,), 6988), ((699050,), 37749864), ((699051,), 35654300), ((1398101,), 71304312),
        ((1398102,), 69208748), ((141120,), 7621976), ((500000,), 27001192), ((1997120,), 98858852),
    ],
    "ls_texture_workspace_bytes": [
        ((1, 1, 1,), 3840), ((2, 16, 16,), 11008), ((1, 1024, 2047,), 37732096), ((1, 1024, 2048,), 37750528),
        ((1, 1025, 2047,), 35671296), ((1, 2048, 2047,), 71270144), ((1, 2048, 2048,), 71304960), ((1, 2049, 2048,), 69242112),
        ((1, 512, 512,), 4719360), ((8, 512, 512,), 37750528), ((8, 1024, 1024,), 138413824),
    ],
}


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_workspace_does_not_grow(name):
    fn = getattr(_native.lib(), name)
    for args, before in BEFORE[name]:
        n = ctypes.c_size_t(0)
        assert fn(*args, ctypes.byref(n)) == 0, (name, args)
        print(name, args, "before", before, "now", n.value)
        assert 0 < n.value <= before, (name, args, n.value, before)
