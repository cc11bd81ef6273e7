/* ORACLE/_ref stand-in (our own text): the reference's precompiled header names <io.h>, which this
 * platform lacks, and uses nothing from it in the code the leaf harness reaches. */
#pragma once
