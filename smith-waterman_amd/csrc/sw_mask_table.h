// sw_mask_table.h -- the one table of the low-complexity mask (sw_db_mask_low_complexity, sw_mask_low_complexity_host; include/swhip.h
// states the rule): G[c] = floor(c x log2(c) x 65536 + 0.5) for c = 0 .. 64, G[0] = G[1] = 0, as integer LITERALS -- never computed at
// run time, so the kernel (csrc/sw_mask.hip) and the host leg (csrc/sw_mask_host.cpp), which both include this file, cannot differ by a
// rounding.  The nearest any c x log2(c) x 65536 comes to a half is 0.0087, far beyond what a double's log2 can err by.  The list is a
// macro so that each side can give it the storage it needs (a constant array on the host, a compile-time table in the kernel).
#pragma once

#define SW_MASK_WINDOW_MAX 64
#define SW_MASK_G_LITERALS                                                                          \
    0, 0, 131072, 311616, 524288, 760849, 1016449, 1287880,                                        \
    1572864, 1869698, 2177059, 2493890, 2819329, 3152656, 3493263, 3840630,                        \
    4194304, 4553891, 4919044, 5289451, 5664838, 6044953, 6429573, 6818492,                        \
    7211522, 7608494, 8009248, 8413640, 8821535, 9232807, 9647339, 10065024,                       \
    10485760, 10909451, 11336007, 11765344, 12197383, 12632049, 13069271, 13508981,                \
    13951115, 14395614, 14842418, 15291475, 15742730, 16196134, 16651639, 17109200,                \
    17568773, 18030316, 18493788, 18959151, 19426369, 19895405, 20366225, 20838795,                \
    21313085, 21789064, 22266701, 22745969, 23226839, 23709285, 24193281, 24678802,                \
    25165824
