/* ORACLE/_ref stand-in (our own text): see cl.h beside this file. */
#pragma once
#include <CL/cl_gl_ext.h>
