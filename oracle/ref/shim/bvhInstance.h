/* ORACLE/_ref stand-in (our own text).  The reference's bvhInstance.h binds a temporary to a
 * non-const reference in one place (its constructor hands a default-constructed 4x4 matrix to
 * SetTransform), which only MSVC accepts.  This file shadows that header on the include path, maps the
 * one constructor-call spelling to a helper that returns a reference to a freshly reset thread-local
 * matrix for exactly the span of the real header, and then includes the real header from where it
 * lies.  Declarations such as 'mat4 x;' or 'mat4& x' are not function-like uses and are untouched. */
#pragma once
inline mat4& ref_leaf_tmp_mat4()
{
	static thread_local mat4 m;
	m = mat4();
	return m;
}
#define mat4( ... ) ref_leaf_tmp_mat4( __VA_ARGS__ )
#include_next "bvhInstance.h"
#undef mat4
