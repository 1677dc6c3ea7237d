/* jpeg_shim.h -- what jpeg_shim.c and jpeg_api.c share (both are part of the libjpeg drop-in, not of the public ABI) */
#ifndef MJH_JPEG_SHIM_H
#define MJH_JPEG_SHIM_H
/* forget the compression in flight on this object, if any (staged image, encoder lease); returns 1 if there was one */
int mjh_shim_drop(void *cinfo);
#ifdef MJH_STANDALONE
/* the decompress half (jpeg_dapi.c): an encoder for these parameters out of the cache the compress half keeps, on the calling
 * thread's device, leased until it is released (NULL: it could not be made, mjh_last_error() says why) */
struct mjh_encoder;
struct mjh_encoder *mjh_shim_cache_acquire(const void *params);
void mjh_shim_cache_release(struct mjh_encoder *enc);
/* forget the image a decompress object holds (jpeg_abort / jpeg_destroy) */
void mjh_dapi_drop(void *cinfo);
#endif
#endif
