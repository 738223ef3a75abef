// Stand-in for GL/glew.h: the OpenGL typedefs and the few enumerants (values of the OpenGL
// registry) that headers of a CUDA/GL interop program mention.  The buffer-object calls do
// nothing; no GL context exists on the host.
#pragma once
#include <stddef.h>
typedef unsigned int GLuint;
typedef int GLint;
typedef unsigned int GLenum;
typedef int GLsizei;
typedef float GLfloat;
typedef unsigned char GLubyte;
typedef unsigned char GLboolean;
typedef ptrdiff_t GLsizeiptr;
#define GL_UNSIGNED_BYTE 0x1401
#define GL_UNSIGNED_SHORT 0x1403
#define GL_FLOAT 0x1406
#define GL_RGB 0x1907
#define GL_RGBA 0x1908
#define GL_LUMINANCE 0x1909
#define GL_LUMINANCE_ALPHA 0x190A
#define GL_BGR 0x80E0
#define GL_BGRA 0x80E1
#define GL_BUFFER_SIZE 0x8764
#define GL_STATIC_DRAW_ARB 0x88E4
#define GL_PIXEL_PACK_BUFFER_ARB 0x88EB
static inline void glBindBuffer(GLenum, GLuint) {}
static inline void glGetBufferParameteriv(GLenum, GLenum, GLint* v) { *v = 0; }
static inline void glBufferData(GLenum, GLsizeiptr, const void*, GLenum) {}
