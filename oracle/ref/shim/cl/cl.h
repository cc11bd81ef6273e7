/* ORACLE/_ref stand-in (our own text): the reference spells its vendored OpenCL header directory in
 * lower case; on a case-sensitive file system it is CL/. */
#pragma once
#include <CL/cl.h>
