// The directional-encoding (IDE) polynomial coefficients as a compile-time table for the device code: term i is
// sum_k kRcIdeCoef[i][k] z^k.  The values are those of build_ide_table (rc_pack_host.h), which stays the one source:
// rc_ide_coef.inc is printed from it by `hostcheck --ide-inc`, and tests/test_ide_constants.py holds the two equal bit
// for bit.  With the term and power loops unrolled a kernel takes the coefficients as immediates; behind a run-time
// index they are scalar loads from constant memory.  Either way nothing of the table is loaded per lane, and the
// compiler need not prove a table in global memory unchanged behind LDS-DMA and asm statements.
#pragma once
#include "rc_pack_host.h"

static constexpr float kRcIdeCoef[RC_IDE_TERMS][RC_IDE_ZPOW] = {
#include "rc_ide_coef.inc"
};
