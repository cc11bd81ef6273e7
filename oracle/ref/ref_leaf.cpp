// ORACLE/_ref (test infrastructure): the reference's own inline leaf code, compiled from the
// headers WHERE THEY LIE and exported as C entry points -- arrays in, arrays out.  Nothing of the
// reference is copied into this repository: this file includes its precompiled header by path at
// build time (as stb_ref.c does for the image loader), and the stand-ins under shim/ declare only
// what that header needs in order to parse on this platform.  Every constructor and member function
// called below is the reference's; this file does no arithmetic of its own except
//   * the six float transcendentals, which follow the project's documented definition
//     (oracle/README.md, "Transcendentals": evaluate in f64, round once to f32) and to which the
//     reference's calls bind through -fno-builtin -Wl,-Bsymbolic (REF_LEAF_LIBM leaves them to libm:
//     the information-only variant of tests/golden/make_ref_leaf_golden.py), and
//   * the random number functions the headers only declare: the documented per-stream xorshift32
//     (Marsaglia 13/17/5) from a seed the caller sets.
// tests/golden/make_ref_leaf_golden.py records its answers in tests/golden/ref_leaf.npz and
// tests/test_ref_leaf_cpu.py holds oracle/, the host mirror and (through the golden) the device to them.
#define _glfw3_native_h_ // GLFW's Win32-native header: nothing of it is used by the headers below
#include "precomp.h"

// ---- what the headers declare and template.cpp would define ------------------------------------
static thread_local uint ref_seed = 0x12345678u;
uint RandomUInt() { ref_seed ^= ref_seed << 13; ref_seed ^= ref_seed >> 17; ref_seed ^= ref_seed << 5; return ref_seed; }
float RandomFloat() { return (float)RandomUInt() * 0x1p-32f; } // [0, 1]: the documented scale, 2^-32
// named from diffuse::scatter, reached only by materials built with raytracer == false; no entry
// point below builds one, and the pin does not extend to template.cpp's rejection sampler
float3 RandomInHemisphere( float3 ) { abort(); }

#ifndef REF_LEAF_LIBM
extern "C" {
float cosf( float x ) noexcept { return (float)cos( (double)x ); }
float sinf( float x ) noexcept { return (float)sin( (double)x ); }
float acosf( float x ) noexcept { return (float)acos( (double)x ); }
float asinf( float x ) noexcept { return (float)asin( (double)x ); }
float expf( float x ) noexcept { return (float)exp( (double)x ); }
float powf( float a, float b ) noexcept { return (float)pow( (double)a, (double)b ); }
}
#endif

// ---- entry points ---------------------------------------------------------------------------------
static inline float3 f3( const float* p ) { return float3( p[0], p[1], p[2] ); }
static inline void put( float* p, const float3& v ) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }
static inline Ray mkray( const float* O, const float* D, float tmax )
{
	Ray r( f3( O ), f3( D ), float3( 0 ), tmax );
	r.hitNormal = float3( 0 ); // the reference leaves it unset until a hit stores one
	r.m = 0;
	return r;
}
static inline void hit_out( const Ray& r, int i, int* hit, float* t, float* nrm )
{
	hit[i] = r.objIdx, t[i] = r.t, put( nrm + 3 * i, r.hitNormal );
}
static const int ID = 7;

extern "C" {

int ref_leaf_libm() {
#ifdef REF_LEAF_LIBM
	return 1;
#else
	return 0;
#endif
}

// Triangle ----------------------------------------------------------------------------------------
void ref_tri_ctor( int n, const float* v9, float* N, float* centroid )
{
	for (int i = 0; i < n; i++) {
		Triangle t( ID, 0, f3( v9 + 9 * i ), f3( v9 + 9 * i + 3 ), f3( v9 + 9 * i + 6 ) );
		put( N + 3 * i, t.N ), put( centroid + 3 * i, t.centroid );
	}
}
void ref_tri_intersect( int n, const float* v9, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm )
{
	for (int i = 0; i < n; i++) {
		Triangle tr( ID, 0, f3( v9 + 9 * i ), f3( v9 + 9 * i + 3 ), f3( v9 + 9 * i + 6 ) );
		Ray r = mkray( O + 3 * i, D + 3 * i, tmax[i] );
		tr.Intersect( r, tmin[i] );
		hit_out( r, i, hit, t, nrm );
	}
}
// IsOccluding has a path with no return statement (edge tests pass, t outside the range); this file is
// built with -fno-strict-return so that the path returns an unspecified value where it would
// otherwise trap.  The callers treat 'true here, but Intersect missed' as that path.
void ref_tri_occluding( int n, const float* v9, const float* O, const float* D, const float* tmax, const float* tmin, int* occ )
{
	for (int i = 0; i < n; i++) {
		Triangle tr( ID, 0, f3( v9 + 9 * i ), f3( v9 + 9 * i + 3 ), f3( v9 + 9 * i + 6 ) );
		Ray r = mkray( O + 3 * i, D + 3 * i, tmax[i] );
		occ[i] = tr.IsOccluding( r, tmin[i] ) ? 1 : 0;
	}
}

// Sphere ------------------------------------------------------------------------------------------
void ref_sphere_intersect( int n, const float* pos, const float* rad, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm )
{
	for (int i = 0; i < n; i++) {
		Sphere s( ID, 0, f3( pos + 3 * i ), rad[i] );
		Ray r = mkray( O + 3 * i, D + 3 * i, tmax[i] );
		s.Intersect( r, tmin[i] );
		hit_out( r, i, hit, t, nrm );
	}
}
void ref_sphere_occluding( int n, const float* pos, const float* rad, const float* O, const float* D, const float* tmax, const float* tmin, int* occ )
{
	for (int i = 0; i < n; i++) {
		Sphere s( ID, 0, f3( pos + 3 * i ), rad[i] );
		Ray r = mkray( O + 3 * i, D + 3 * i, tmax[i] );
		occ[i] = s.IsOccluding( r, tmin[i] ) ? 1 : 0;
	}
}
void ref_sphere_normal( int n, const float* pos, const float* rad, const float* I, float* nrm )
{
	for (int i = 0; i < n; i++) {
		Sphere s( ID, 0, f3( pos + 3 * i ), rad[i] );
		put( nrm + 3 * i, s.GetNormal( f3( I + 3 * i ) ) );
	}
}

// Plane -------------------------------------------------------------------------------------------
void ref_plane_intersect( int n, const float* N, const float* d, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm )
{
	for (int i = 0; i < n; i++) {
		Plane p( ID, 0, f3( N + 3 * i ), d[i] );
		Ray r = mkray( O + 3 * i, D + 3 * i, tmax[i] );
		p.Intersect( r, tmin[i] );
		hit_out( r, i, hit, t, nrm );
	}
}
void ref_plane_occluding( int n, const float* N, const float* d, const float* O, const float* D, const float* tmax, const float* tmin, int* occ )
{
	for (int i = 0; i < n; i++) {
		Plane p( ID, 0, f3( N + 3 * i ), d[i] );
		Ray r = mkray( O + 3 * i, D + 3 * i, tmax[i] );
		occ[i] = p.IsOccluding( r, tmin[i] ) ? 1 : 0;
	}
}

// AreaLight ---------------------------------------------------------------------------------------
// light[i*12..]: pos(3) strength col(3) radius normal(3) raytracer
static inline AreaLight mkarea( const float* L ) { return AreaLight( ID, f3( L ), L[3], f3( L + 4 ), L[7], f3( L + 8 ), 4, L[11] != 0 ); }
void ref_area_intersect( int n, const float* L, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm )
{
	for (int i = 0; i < n; i++) {
		AreaLight a = mkarea( L + 12 * i );
		Ray r = mkray( O + 3 * i, D + 3 * i, tmax[i] );
		a.Intersect( r, tmin[i] );
		hit_out( r, i, hit, t, nrm );
	}
}
void ref_area_intensity( int n, const float* L, const float* p, const float* nrm, const float* from, float* rgb )
{
	for (int i = 0; i < n; i++) {
		AreaLight a = mkarea( L + 12 * i );
		put( rgb + 3 * i, a.GetLightIntensityAt( f3( p + 3 * i ), f3( nrm + 3 * i ), f3( from + 3 * i ) ) );
	}
}
void ref_area_position( int n, const float* L, const unsigned* seedIn, float* pos, unsigned* seedOut )
{
	for (int i = 0; i < n; i++) {
		AreaLight a = mkarea( L + 12 * i );
		ref_seed = seedIn[i];
		put( pos + 3 * i, a.GetLightPosition() );
		seedOut[i] = ref_seed;
	}
}

// DirectionalLight --------------------------------------------------------------------------------
// light[i*8..]: pos(3) strength normal(3) r
static inline DirectionalLight mkdir( const float* L ) { return DirectionalLight( ID, f3( L ), L[3], float3( 1 ), f3( L + 4 ), L[7], true ); }
void ref_dir_ctor( int n, const float* L, float* sinAngle )
{
	for (int i = 0; i < n; i++) sinAngle[i] = mkdir( L + 8 * i ).sinAngle;
}
void ref_dir_intensity( int n, const float* L, const float* p, float* rgb )
{
	for (int i = 0; i < n; i++) {
		DirectionalLight d = mkdir( L + 8 * i );
		put( rgb + 3 * i, d.GetLightIntensityAt( f3( p + 3 * i ), float3( 0, 1, 0 ), float3( 0 ) ) );
	}
}

// glass -------------------------------------------------------------------------------------------
void ref_glass_fresnel( int n, const float* I, const float* N, const float* ior, float* kr )
{
	glass g( 1.5f, float3( 1 ), float3( 0 ), 0, 0, true );
	for (int i = 0; i < n; i++) {
		float k = 0;
		g.fresnel( f3( I + 3 * i ), f3( N + 3 * i ), ior[i], k );
		kr[i] = k;
	}
}
void ref_glass_refract( int n, const float* D, const float* N, const float* ratio, float* out )
{
	glass g( 1.5f, float3( 1 ), float3( 0 ), 0, 0, true );
	for (int i = 0; i < n; i++) put( out + 3 * i, g.RefractRay( f3( D + 3 * i ), f3( N + 3 * i ), ratio[i] ) );
}

// diffuse::scatter of a material built with raytracer == true (draws nothing; the scattered ray's
// direction is left unset by the reference and is not reported) and metal::scatter --------------------
// m[i*6..]: albedo(3) ks kd n
void ref_diffuse_scatter( int n, const float* m, const float* O, const float* D, const float* t, const float* lightDir, const float* lightInt,
                          const float* nrm, const float* energyIn, float* att, float* energyOut, float* scatO )
{
	for (int i = 0; i < n; i++) {
		const float* M = m + 6 * i;
		diffuse d( f3( M ), float3( 1 ), M[3], M[4], (int)M[5], true );
		Ray r = mkray( O + 3 * i, D + 3 * i, t[i] ), s;
		float3 a( 0 ), e = f3( energyIn + 3 * i );
		d.scatter( r, a, s, f3( lightDir + 3 * i ), f3( lightInt + 3 * i ), f3( nrm + 3 * i ), e );
		put( att + 3 * i, a ), put( energyOut + 3 * i, e ), put( scatO + 3 * i, s.O );
	}
}
void ref_metal_scatter( int n, const float* O, const float* D, const float* t, const float* nrm, float* outO, float* outD, int* ret )
{
	metal m( 0.7f, float3( 1 ), true );
	for (int i = 0; i < n; i++) {
		Ray r = mkray( O + 3 * i, D + 3 * i, t[i] ), s;
		float3 e( 1 );
		ret[i] = m.scatter( r, s, f3( nrm + 3 * i ), e ) ? 1 : 0;
		put( outO + 3 * i, s.O ), put( outD + 3 * i, s.D );
	}
}

// Camera::GetPrimaryRay at the reference's fixed screen size -------------------------------------------
// cam: camPos(3) topLeft(3) topRight(3) bottomLeft(3) fishEye viewAngle yAngle
int ref_camera_width() { return SCRWIDTH; }
int ref_camera_height() { return SCRHEIGHT; }
void ref_camera_default( float* cam )
{
	Camera c;
	put( cam, c.camPos ), put( cam + 3, c.topLeft ), put( cam + 6, c.topRight ), put( cam + 9, c.bottomLeft );
	cam[12] = c.fishEye, cam[13] = c.viewAngle, cam[14] = c.yAngle;
}
void ref_camera_rays( const float* cam, int n, const int* xs, const int* ys, float* O, float* D )
{
	Camera c;
	c.camPos = f3( cam ), c.topLeft = f3( cam + 3 ), c.topRight = f3( cam + 6 ), c.bottomLeft = f3( cam + 9 );
	c.screenCenter = c.topLeft + .5f * (c.topRight - c.topLeft) + .5f * (c.bottomLeft - c.topLeft); // what every mover of the camera ends with
	c.fishEye = cam[12] != 0, c.viewAngle = cam[13], c.yAngle = cam[14];
	for (int i = 0; i < n; i++) {
		Ray r = c.GetPrimaryRay( xs[i], ys[i] );
		put( O + 3 * i, r.O ), put( D + 3 * i, r.D );
	}
}

// Scene::GetSkyColor.  A Scene cannot be constructed (its constructor builds a BVH: bvh.cpp), and the
// function reads only four plain members, so it runs on zeroed storage with those four set.
void ref_sky_color( int w, int h, int nch, const unsigned char* px, int n, const float* D, float* rgb )
{
	Scene* s = (Scene*)calloc( 1, sizeof( Scene ) );
	s->skydome = (unsigned char*)px, s->skydomeX = w, s->skydomeY = h, s->skydomeN = nch;
	for (int i = 0; i < n; i++) {
		Ray r = mkray( D + 3 * i, D + 3 * i, 1e34f );
		put( rgb + 3 * i, s->GetSkyColor( r ) );
	}
	free( s );
}

} // extern "C"
