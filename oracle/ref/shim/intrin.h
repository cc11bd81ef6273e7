/* ORACLE/_ref stand-in (our own text): MSVC's <intrin.h> is <x86intrin.h> here. */
#pragma once
#include <x86intrin.h>
