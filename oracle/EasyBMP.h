// Stand-in for the bitmap library the reference program expects as a third-party
// header.  The oracle build only needs the reference's bitmap dumper and loader to
// compile; recorded fixtures are full-precision DAT files, never images.  This
// class keeps no pixels and writes nothing.
#ifndef ORACLE_EASYBMP_STANDIN_H
#define ORACLE_EASYBMP_STANDIN_H

typedef unsigned char ebmpBYTE;

struct RGBApixel
{
  ebmpBYTE Blue, Green, Red, Alpha;
  RGBApixel () : Blue (0), Green (0), Red (0), Alpha (0) {}
};

class BMP
{
  int width, height, depth;

public:
  BMP () : width (1), height (1), depth (24) {}

  bool SetSize (int w, int h) { width = w; height = h; return true; }
  bool SetBitDepth (int d) { depth = d; return true; }
  int TellWidth () const { return width; }
  int TellHeight () const { return height; }
  int TellBitDepth () const { return depth; }

  RGBApixel GetPixel (int, int) const { return RGBApixel (); }
  bool SetPixel (int, int, RGBApixel) { return true; }
  RGBApixel *operator() (int, int) { static RGBApixel scratch; return &scratch; }

  bool WriteToFile (const char *) { return true; }
  bool ReadFromFile (const char *) { return false; }
};

#endif
