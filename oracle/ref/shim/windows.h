/* ORACLE/_ref stand-in (our own text): just enough of "windows.h" for the reference's precompiled
 * header to parse.  The three types are only members of its job-manager classes, which the leaf
 * harness never constructs; the two C headers are what the real one pulls in as a side effect. */
#pragma once
#include <string.h>
#include <stdlib.h>
typedef void* HANDLE;
typedef struct { void* opaque[5]; } CRITICAL_SECTION;
typedef union { struct { unsigned int LowPart; int HighPart; } u; long long QuadPart; } LARGE_INTEGER;
