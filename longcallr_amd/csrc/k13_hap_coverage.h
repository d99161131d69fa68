// k13_hap_coverage.h — the one size of K13 (k13_hap_coverage.hip) that its tests read.
#pragma once

// Window columns a workgroup scans and compacts per step: LCR_BLOCK threads x 4 consecutive columns.  A region's workgroup walks its
// window in steps of this many columns and carries the three running depths, and the running segment rank, from one step into the next.
#define K13_TILE 1024
